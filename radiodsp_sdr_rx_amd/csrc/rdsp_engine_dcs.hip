/*
 * rdsp_engine_dcs.hip -- rdsp_engine_t's DCS code squelch (include/rdsp.h has the definition, rdsp_dcs.h the arithmetic): the
 * kernel an NFM group launches behind its tone-squelch kernel (behind its meter kernel without one).  It reads the group's
 * demodulated rows once, writes three records a block and, with the meter on, closes the blocks the gates in front of it left
 * open that do not carry the receiver's code.  Compiled with the engine's flags (-ffp-contract=off).
 *
 * rdsp_engine_dcs_kernel has the meter kernel's shape: one wave per channel, four channels a workgroup, no table and no barrier;
 * a wave past the last channel leaves at once.  Eight blocks a trip, loaded and decimated as the tone search does: a half-wave
 * holds a block, lane l of 32 loads samples 4 l ... 4 l + 3 in one 16-byte load and adds them as levels 1 and 2 of the tree, the
 * exchanges with strides 1, 2 (quad permutes) and 4 (row_half_mirror) are levels 3 ... 5.  The trip's 32 decimated values then
 * reach every lane wave-uniformly, in order.  Lane p of 0 ... 7 IS hypothesis p: its acc, pos, nb, hits and last live in its
 * registers across the call; the eight rings lie in LDS, 8 x 23 floats a wave, indexed by pos.  A wave's LDS accesses execute in
 * order, so between its own writes and reads a wavefront-scope fence is all that is needed (wg_sync<1>).  Which hypothesis ticks
 * is wave-uniform (dcs_tick).  On a tick the lane of the hypothesis stores acc, every lane adds the ring left to right (uniform
 * reads), lane j of 0 ... 22 slices bit j and a ballot is the word; lane r of 0 ... 22 then tests rotation r and a second ballot
 * is the match; canon of a word read under ANY is a butterfly minimum.  The end of a window is wave-uniform.  Lane j keeps block
 * j's records and lanes 0 ... 7 write them; a block the code closes has its 128 audio words overwritten with zeros by the
 * half-wave that held it, 16 bytes a lane.  A channel without a code writes zero words and zero records and leaves the gate alone.
 */
#include <hip/hip_runtime.h>

#include "rdsp_engine_dcs.h"
#include "rdsp_engine_meter.h"
#include "rdsp_wave.h"

using namespace rdsp_eng;
using namespace rdsp_dcs;

namespace {
constexpr int DW = 256, DCH = DW / 64; /* the meter's workgroup: four waves, four channels */
constexpr int DSTEP = 8;               /* blocks in flight per wave */

/* levels 3 ... 5 of the tree over eight lanes, the result in every one of them: the tone search's exchange */
__device__ __forceinline__ float oct_allsum(float v) {
  v += dpp_f<0xB1>(v);  /* quad_perm [1,0,3,2] */
  v += dpp_f<0x4E>(v);  /* quad_perm [2,3,0,1] */
  v += dpp_f<0x141>(v); /* row_half_mirror */
  return v;
}
__device__ __forceinline__ float lane_value(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
__device__ __forceinline__ uint32_t lane_word(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }
__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
/* the smallest of the 23 rotations, wave-uniform: lane r holds rotation r */
__device__ __forceinline__ uint32_t wave_canon(uint32_t w, int lane) {
  uint32_t m = lane < BITS ? dcs_rot(w, lane) : 0xFFFFFFFFu;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)m, s);
    m = o < m ? o : m;
  }
  return uniform(m);
}
}  // namespace

__global__ __launch_bounds__(DW) void rdsp_engine_dcs_kernel(const DcsParams p) {
  const int lane = (int)threadIdx.x & 63, half = lane >> 5, l32 = lane & 31, wave = (int)threadIdx.x >> 6;
  const int ch = (int)blockIdx.x * DCH + wave;
  __shared__ float rings[DCH][HYP * BITS];
  if (ch >= p.n_channels) return;
  uint32_t *w = p.state + (size_t)ch * DCS_WORDS;
  uint8_t *dcs_rec = p.dcs + (size_t)ch * p.rec_stride, *hits_rec = p.hits + (size_t)ch * p.rec_stride;
  uint32_t *word_rec = p.word + (size_t)ch * p.rec_stride;
  const uint32_t sel = uniform(p.sel[ch]);
  if (sel == 0u) { /* no code: zero words, zero records, the gate is the others' */
    for (int b = lane; b < p.n_blocks; b += 64) { dcs_rec[b] = 0; hits_rec[b] = 0; word_rec[b] = 0u; }
    for (int i = lane; i < DCS_WORDS; i += 64) w[i] = 0u;
    return;
  }
  const DcsLaw law = p.law;
  const uint32_t key = dcs_key(sel, law.max_err), want = key & WORD_MASK;
  const bool any_code = (key & KEY_ANY) != 0u;
  /* the detector the call begins with: zeros behind a reset, another key or another K */
  const bool fresh = p.reset != 0 || uniform(w[DC_KEY]) != key || uniform(w[DC_K]) != law.K;
  uint32_t cnt = fresh ? 0u : uniform(w[DC_CNT]), dcs = fresh ? 0u : uniform(w[DC_DCS]), H = fresh ? 0u : uniform(w[DC_H]);
  uint32_t word = fresh ? 0u : uniform(w[DC_WORD]), ms = fresh ? 0u : uniform(w[DC_MS]);
  float *ring = rings[wave];
  for (int i = lane; i < HYP * BITS; i += 64)
    ring[i] = fresh ? 0.0f : __uint_as_float(w[DC_HYP + (i / BITS) * HYP_WORDS + DH_RING + i % BITS]);
  float acc = 0.0f;
  uint32_t pos = 0u, nb = 0u, hits = 0u, last = 0u;
  if (!fresh && lane < HYP) {
    const uint32_t *h = w + DC_HYP + lane * HYP_WORDS;
    acc = __uint_as_float(h[DH_ACC]); pos = h[DH_POS]; nb = h[DH_NB]; hits = h[DH_HITS]; last = h[DH_LAST];
    if (pos >= (uint32_t)BITS) pos = 0u; /* words no detector wrote: stay inside the ring */
  }
  const uint32_t canon_want = any_code ? 0u : wave_canon(want, lane);
  wg_sync<1>(); /* the rings are filled */
  const float4 *row = (const float4 *)(p.audio + (size_t)ch * p.audio_stride);
  const bool gated = p.open != nullptr;
  uint8_t *open_rec = gated ? p.open + (size_t)ch * p.open_stride : nullptr;
  int32_t *out = p.out + (size_t)ch * p.out_stride;
  int any = 0;
  for (int b0 = 0; b0 < p.n_blocks; b0 += DSTEP) {
    float d[DSTEP / 2];
#pragma unroll
    for (int k = 0; k < DSTEP / 2; k++) {
      const int b = b0 + 2 * k + half;
      const float4 v = b < p.n_blocks ? row[(size_t)b * (BLOCK / 4) + l32] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      d[k] = oct_allsum(rdsp_tone_search::search_quad(v.x, v.y, v.z, v.w));
    }
    int was_open = 0; /* lane j: the record of block b0 + j the gates in front left */
    if (gated && lane < DSTEP && b0 + lane < p.n_blocks) was_open = open_rec[b0 + lane];
    uint32_t rec_dcs = 0u, rec_hits = 0u, rec_word = 0u;
    int rec_open = 0;
#pragma unroll
    for (int j = 0; j < DSTEP; j++) {
      if (b0 + j < p.n_blocks) { /* wave-uniform */
#pragma unroll
        for (int q = 0; q < PER_BLOCK; q++) {
          acc = acc + lane_value(d[j >> 1], 32 * (j & 1) + 8 * q);
          ms += law.step;
          const int pt = dcs_tick(ms, law.step);
          if (pt >= 0) { /* wave-uniform: hypothesis pt ticks */
            float *rg = ring + pt * BITS;
            const uint32_t pos0 = lane_word(pos, pt), pos1 = pos0 + 1u == (uint32_t)BITS ? 0u : pos0 + 1u;
            const uint32_t nb0 = lane_word(nb, pt), nb1 = nb0 + 1u < (uint32_t)BITS ? nb0 + 1u : (uint32_t)BITS;
            if (lane == pt) { rg[pos0] = acc; acc = 0.0f; pos = pos1; nb = nb1; }
            wg_sync<1>();
            const float thr = dcs_thr(rg);
            const uint32_t at = pos1 + (uint32_t)lane;
            const bool one = lane < BITS && rg[at >= (uint32_t)BITS ? at - (uint32_t)BITS : at] > thr;
            const uint32_t wd = (uint32_t)__ballot(one) & WORD_MASK;
            wg_sync<1>();
            if (nb1 == (uint32_t)BITS) {
              bool match;
              uint32_t matched = canon_want;
              if (any_code) {
                match = dcs_any_word(wd) && __ballot(lane < BITS && dcs_any_rot(wd, lane)) != 0ull;
                if (match) matched = wave_canon(wd, lane);
              } else {
                match = __ballot(lane < BITS && dcs_code_rot(wd, want, lane, law.max_err)) != 0ull;
              }
              if (match && lane == pt) { hits += 1u; last = matched; }
            }
          }
        }
        cnt += 1u;
        if (cnt == law.K) { /* wave-uniform: the window's end */
          int best = 0;
          H = lane_word(hits, 0);
#pragma unroll
          for (int q = 1; q < HYP; q++) {
            const uint32_t h = lane_word(hits, q);
            if (h > H) { H = h; best = q; }
          }
          dcs = dcs_decide(H, dcs, law);
          word = H ? lane_word(last, best) : 0u;
          hits = 0u; last = 0u; cnt = 0u;
        }
        if (lane == j) { rec_dcs = dcs; rec_hits = H; rec_word = word; }
        if (gated) {
          const int before = __builtin_amdgcn_readlane(was_open, j), both = before & (int)dcs;
          any |= both;
          if (lane == j) rec_open = both;
          if (before && !both && half == (j & 1)) { /* newly closed: the half-wave that held the block */
            int32_t *o = out + (size_t)(b0 + j) * BLOCK + 4 * l32;
            if (p.out_vec) *(int4 *)o = make_int4(0, 0, 0, 0);
            else { o[0] = 0; o[1] = 0; o[2] = 0; o[3] = 0; }
          }
        }
      }
    }
    if (lane < DSTEP && b0 + lane < p.n_blocks) {
      dcs_rec[b0 + lane] = (uint8_t)rec_dcs; hits_rec[b0 + lane] = (uint8_t)rec_hits; word_rec[b0 + lane] = rec_word;
      if (gated) open_rec[b0 + lane] = (uint8_t)rec_open;
    }
  }
  wg_sync<1>();
  for (int i = lane; i < HYP * BITS; i += 64) w[DC_HYP + (i / BITS) * HYP_WORDS + DH_RING + i % BITS] = __float_as_uint(ring[i]);
  if (lane < HYP) {
    uint32_t *h = w + DC_HYP + lane * HYP_WORDS;
    h[DH_ACC] = __float_as_uint(acc); h[DH_POS] = pos; h[DH_NB] = nb; h[DH_HITS] = hits; h[DH_LAST] = last;
  }
  if (lane == 0) {
    w[DC_KEY] = key; w[DC_K] = law.K; w[DC_CNT] = cnt; w[DC_DCS] = dcs; w[DC_H] = H; w[DC_WORD] = word; w[DC_MS] = ms; w[7] = 0u;
    if (gated) p.meter_words[(size_t)ch * MT_WORDS + MT_ANY] = __int_as_float(any);
  }
}

hipError_t rdsp_engine_dcs_launch(const DcsParams &p, hipStream_t s) {
  if (p.n_channels < 1 || p.n_blocks < 1) return hipSuccess;
  hipLaunchKernelGGL(rdsp_engine_dcs_kernel, dim3((unsigned)((p.n_channels + DCH - 1) / DCH)), dim3(DW), 0, s, p);
  return hipGetLastError();
}
