/*
 * rdsp_engine_meter.hip -- rdsp_engine_t's signal meter, squelch gate and active-receiver list (include/rdsp.h has the
 * definition, rdsp_meter.h the arithmetic).  Compiled with the engine's flags (-ffp-contract=off).
 *
 * rdsp_engine_meter_kernel, per group behind the group's tail kernel: one wave per channel, four channels a workgroup, no
 * LDS, no barrier (a wave past the last channel leaves at once).  A half-wave holds one block: lane l of 32 loads samples
 * 4 l ... 4 l + 3 in one 16-byte load (a wave's load is two consecutive blocks, 1 KiB, coalesced), squares and adds them as
 * levels 1 and 2 of the tree, and the 32 lanes exchange with strides 1, 2 (quad permutes), 4, 8 (row mirrors: the lanes of a
 * quad, then of a half row, already hold the same sum) and 16 (a swizzle inside the half-wave): levels 3 ... 7.  Eight blocks
 * are loaded before the first is reduced.  The level and gate recursions then run wave-uniform over those blocks in block
 * order; lane j keeps block j's record and lanes 0 ... 7 write them; a closed block's 128 audio words are overwritten with
 * zeros by the half-wave that held it, 16 bytes a lane.
 * rdsp_engine_active_kernel, once per call: one workgroup walks the channels in ascending chunks of 1024; inside a chunk a
 * wave's ballot gives every open channel its place among the wave's, the waves' counts are added in wave order, and the chunks'
 * in chunk order -- an ordered scan, no atomics: the list is ascending by construction.
 */
#include <hip/hip_runtime.h>

#include "rdsp_engine_meter.h"
#include "rdsp_wave.h"

using namespace rdsp_eng;
using namespace rdsp_meter;

namespace {
constexpr int MW = 256, MCH = MW / 64; /* the meter's workgroup: four waves, four channels */
constexpr int MSTEP = 8;               /* blocks in flight per wave */
constexpr int AW = 1024;               /* the list's workgroup */

__device__ __forceinline__ float swap16(float v) { /* lane ^ 16 inside each 32 lanes: and 0x1f, or 0, xor 0x10 */
  return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x401F));
}
/* levels 3 ... 7 of the tree over the 32 lanes of a half-wave, the result in every one of them */
__device__ __forceinline__ float half_allsum(float v) {
  v += dpp_f<0xB1>(v);  /* quad_perm [1,0,3,2] */
  v += dpp_f<0x4E>(v);  /* quad_perm [2,3,0,1] */
  v += dpp_f<0x141>(v); /* row_half_mirror */
  v += dpp_f<0x140>(v); /* row_mirror */
  v += swap16(v);
  return v;
}
__device__ __forceinline__ float half_allmax(float v) {
  v = fmaxf(v, dpp_f<0xB1>(v));
  v = fmaxf(v, dpp_f<0x4E>(v));
  v = fmaxf(v, dpp_f<0x141>(v));
  v = fmaxf(v, dpp_f<0x140>(v));
  v = fmaxf(v, swap16(v));
  return v;
}
__device__ __forceinline__ float lane_value(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
}  // namespace

__global__ __launch_bounds__(MW) void rdsp_engine_meter_kernel(const MeterParams p) {
  const int lane = (int)threadIdx.x & 63, half = lane >> 5, l32 = lane & 31;
  const int ch = (int)blockIdx.x * MCH + ((int)threadIdx.x >> 6);
  if (ch >= p.n_channels) return;
  const float4 *row = (const float4 *)(p.audio + (size_t)ch * p.audio_stride);
  int32_t *out = p.out + (size_t)ch * p.out_stride;
  float *w = p.words + (size_t)ch * MT_WORDS;
  MeterState g;
  g.level = w[MT_LEVEL]; g.open = __float_as_int(w[MT_OPEN]); g.hang = __float_as_int(w[MT_HANG]);
  int any = 0;
  float ms = 0.0f, pk = 0.0f;
  for (int b0 = 0; b0 < p.n_blocks; b0 += MSTEP) {
    float4 v[MSTEP / 2];
#pragma unroll
    for (int k = 0; k < MSTEP / 2; k++) {
      const int b = b0 + 2 * k + half;
      v[k] = b < p.n_blocks ? row[(size_t)b * (BLOCK / 4) + l32] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    float sum[MSTEP / 2], top[MSTEP / 2];
#pragma unroll
    for (int k = 0; k < MSTEP / 2; k++) {
      sum[k] = half_allsum(quad_sum(v[k].x, v[k].y, v[k].z, v[k].w));
      top[k] = half_allmax(quad_peak(v[k].x, v[k].y, v[k].z, v[k].w));
    }
    float rec_level = 0.0f, rec_peak = 0.0f;
    int rec_open = 0;
#pragma unroll
    for (int j = 0; j < MSTEP; j++) {
      if (b0 + j < p.n_blocks) { /* wave-uniform */
        ms = mean_square(lane_value(sum[j >> 1], 32 * (j & 1)));
        pk = lane_value(top[j >> 1], 32 * (j & 1));
        g.level = level_step(g.level, ms, p.set.attack, p.set.decay);
        gate_step(g, p.set);
        any |= g.open;
        if (lane == j) { rec_level = g.level; rec_peak = pk; rec_open = g.open; }
        if (!g.open && half == (j & 1)) { /* the half-wave that held the block */
          int32_t *o = out + (size_t)(b0 + j) * BLOCK + 4 * l32;
          if (p.out_vec) *(int4 *)o = make_int4(0, 0, 0, 0);
          else { o[0] = 0; o[1] = 0; o[2] = 0; o[3] = 0; }
        }
      }
    }
    if (lane < MSTEP && b0 + lane < p.n_blocks) {
      const size_t at = (size_t)ch * p.rec_stride + (size_t)(b0 + lane);
      p.level[at] = rec_level; p.peak[at] = rec_peak; p.open[at] = (uint8_t)rec_open;
    }
  }
  if (lane == 0) {
    w[MT_LEVEL] = g.level; w[MT_OPEN] = __int_as_float(g.open); w[MT_HANG] = __int_as_float(g.hang);
    w[MT_LAST_MS] = ms; w[MT_LAST_PK] = pk; w[MT_ANY] = __int_as_float(any);
  }
}

__global__ __launch_bounds__(AW) void rdsp_engine_active_kernel(const ActiveParams p) {
  __shared__ int wave_count[AW / 64];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int base = 0;
  for (int c0 = 0; c0 < p.n_channels; c0 += AW) { /* the same trips for every thread */
    const int c = c0 + tid;
    const bool on = c < p.n_channels && __float_as_int(p.words[(size_t)c * MT_WORDS + MT_ANY]) != 0;
    const unsigned long long ballot = __ballot(on);
    if (lane == 0) wave_count[wave] = __popcll(ballot);
    __syncthreads();
    int before = base, total = 0;
    for (int k = 0; k < AW / 64; k++) {
      if (k < wave) before += wave_count[k];
      total += wave_count[k];
    }
    if (on) p.list[before + __popcll(ballot & ((1ull << lane) - 1ull))] = c;
    base += total;
    __syncthreads(); /* wave_count is written again */
  }
  if (tid == 0) *p.count = base;
}

hipError_t rdsp_engine_meter_launch(const MeterParams &p, hipStream_t s) {
  if (p.n_channels < 1 || p.n_blocks < 1) return hipSuccess;
  hipLaunchKernelGGL(rdsp_engine_meter_kernel, dim3((unsigned)((p.n_channels + MCH - 1) / MCH)), dim3(MW), 0, s, p);
  return hipGetLastError();
}
hipError_t rdsp_engine_active_launch(const ActiveParams &p, hipStream_t s) {
  hipLaunchKernelGGL(rdsp_engine_active_kernel, dim3(1), dim3(AW), 0, s, p);
  return hipGetLastError();
}
