/*
 * rdsp_engine_noise.hip -- rdsp_engine_t's noise squelch (include/rdsp.h has the definition, rdsp_noise.h the arithmetic): the
 * kernel an NFM group launches behind its meter kernel, in front of its tone kernel.  It reads the group's demodulated rows once,
 * writes two records a block and, at mode 2 with the meter on, closes the blocks the carrier gate left open whose discriminator
 * noise says "no station".  Compiled with the engine's flags (-ffp-contract=off).
 *
 * rdsp_engine_noise_kernel has the tone kernel's shape: one wave per channel, four channels a workgroup, eight blocks a trip, a
 * half-wave per block; no workgroup barrier (a wave past the last channel leaves at once, the LDS of a wave is its own, and
 * between its own writes and reads a wavefront-scope fence is all that is needed: wg_sync<1>).  The wave stages the trip's 1024
 * floats behind the 64 carried ones in its region of LDS, 4352 bytes: lane l of a half-wave stores samples 4 l ... 4 l + 3 of its
 * block with one 16-byte store.  Output j of a block needs the 65 samples a[4 j + 3 - 64 ... 4 j + 3]: with the block at float4
 * 16 + 32 blk of the region they are the last 65 words of the 17 float4 from 32 blk + j on, so lane j reads whole aligned float4
 * and consecutive lanes' windows lie 16 bytes apart.  The taps are kernel arguments: they arrive through the constant address
 * space in scalar registers.  Four chains a lane (its half-wave's four blocks of the trip) run side by side, k ascending as the
 * definition has it; then the square and the five exchanges of the meter's tree over the 32 lanes.  The level and gate recursion
 * runs wave-uniform over the trip's blocks in order; lane j keeps block j's records and lanes 0 ... 7 write them; a block the gate
 * closes has its 128 audio words overwritten with zeros by the half-wave that held it, 16 bytes a lane.  The last 64 samples of a
 * trip move to the front of the region for the next one and, behind the last, into the channel's words.
 */
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "rdsp_engine_meter.h"
#include "rdsp_engine_noise.h"
#include "rdsp_wave.h"

using namespace rdsp_eng;
using namespace rdsp_noise;

namespace {
constexpr int NW = 256, NCH = NW / 64; /* the meter's workgroup: four waves, four channels */
constexpr int NSTEP = 8;               /* blocks in flight per wave */
constexpr int LEAD4 = NOISE_HIST / 4;  /* float4 in front of a trip's first sample */
constexpr int REGION4 = LEAD4 + NSTEP * BLOCK / 4;
constexpr int WIN4 = NOISE_PROTO / 4 + 1; /* a window's 65 words end a run of 17 float4 */

__device__ __forceinline__ float swap16(float v) { /* lane ^ 16 inside each 32 lanes: and 0x1f, or 0, xor 0x10 */
  return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x401F));
}
/* the five levels of the tree over the 32 lanes of a half-wave, the result in every one of them: the meter's exchange */
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

typedef const __attribute__((address_space(4))) float *ConstTaps;
/* the taps where they arrive: the kernel's one argument lies at the start of the kernel-argument segment */
__device__ __forceinline__ ConstTaps arg_taps() {
  return (ConstTaps)((const __attribute__((address_space(4))) char *)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(NoiseParams, taps));
}
}  // namespace

__global__ __launch_bounds__(NW) void rdsp_engine_noise_kernel(const NoiseParams p) {
  const int lane = (int)threadIdx.x & 63, half = lane >> 5, l32 = lane & 31, wave = (int)threadIdx.x >> 6;
  const int ch = (int)blockIdx.x * NCH + wave;
  __shared__ float4 region[NCH][REGION4];
  if (ch >= p.n_channels) return;
  float4 *x4 = region[wave];
  float *x = (float *)x4;
  uint32_t *w = p.state + (size_t)ch * NOISE_WORDS;
  float *noise_rec = p.noise + (size_t)ch * p.rec_stride;
  uint8_t *nopen_rec = p.nopen + (size_t)ch * p.rec_stride;
  NoiseState st;
  st.key = uniform(w[NZ_KEY]); st.N = __uint_as_float(uniform(w[NZ_N]));
  st.open = (int32_t)uniform(w[NZ_OPEN]); st.hang = (int32_t)uniform(w[NZ_HANG]);
  const bool fresh = noise_start(st, p.key, p.reset != 0);
  x[lane] = fresh ? 0.0f : __uint_as_float(w[NZ_HIST + lane]); /* NOISE_HIST is the wave's 64 lanes */
  const float4 *row = (const float4 *)(p.audio + (size_t)ch * p.audio_stride);
  const bool gated = p.open != nullptr;
  uint8_t *open_rec = gated ? p.open + (size_t)ch * p.open_stride : nullptr;
  int32_t *out = p.out + (size_t)ch * p.out_stride;
  int any = 0;
  for (int b0 = 0; b0 < p.n_blocks; b0 += NSTEP) {
    /* the taps are loaded anew every trip, sixteen at a time in front of their use: all 65 held across the loop do not fit
     * the scalar registers beside the rest */
    ConstTaps t = arg_taps();
    asm volatile("" : "+s"(t));
#pragma unroll
    for (int k = 0; k < NSTEP / 2; k++) {
      const int b = b0 + 2 * k + half;
      x4[LEAD4 + (2 * k + half) * (BLOCK / 4) + l32] = b < p.n_blocks ? row[(size_t)b * (BLOCK / 4) + l32] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    int was_open = 0; /* lane j: the carrier gate's record of block b0 + j */
    if (gated && lane < NSTEP && b0 + lane < p.n_blocks) was_open = open_rec[b0 + lane];
    wg_sync<1>(); /* the trip is staged behind the carried samples */
    float v[NSTEP / 2] = {0.0f, 0.0f, 0.0f, 0.0f};
    /* tap k of output j is word 67 - k of the lane's 17 float4: float4 f holds taps 64 - 4 f (its last word) ... 67 - 4 f */
#pragma unroll
    for (int f = WIN4 - 1; f >= 1; f--) {
      const int k0 = NOISE_PROTO - 4 * f;
      const float g0 = t[k0], g1 = t[k0 + 1], g2 = t[k0 + 2], g3 = t[k0 + 3];
#pragma unroll
      for (int k = 0; k < NSTEP / 2; k++) {
        const float4 q = x4[(2 * k + half) * (BLOCK / 4) + l32 + f];
        v[k] = noise_mac(noise_mac(noise_mac(noise_mac(v[k], g0, q.w), g1, q.z), g2, q.y), g3, q.x);
      }
      /* sixteen float4 in flight, not all 68: the scheduler would hoist every read of the window, 150 VGPRs and three waves a SIMD */
      if (f % 4 == 1) __builtin_amdgcn_sched_barrier(0);
    }
    float nz[NSTEP / 2];
#pragma unroll
    for (int k = 0; k < NSTEP / 2; k++) {
      v[k] = noise_mac(v[k], t[NOISE_PROTO], x4[(2 * k + half) * (BLOCK / 4) + l32].w);
      nz[k] = noise_reading(half_allsum(v[k] * v[k]));
    }
    float rec_n = 0.0f;
    int rec_nopen = 0, rec_open = 0;
#pragma unroll
    for (int j = 0; j < NSTEP; j++) {
      if (b0 + j < p.n_blocks) { /* wave-uniform */
        noise_step(st, lane_value(nz[j >> 1], 32 * (j & 1)), p.set);
        if (lane == j) { rec_n = st.N; rec_nopen = st.open; }
        if (gated) {
          const int carrier = __builtin_amdgcn_readlane(was_open, j), both = carrier & st.open;
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
    if (lane < NSTEP && b0 + lane < p.n_blocks) {
      noise_rec[b0 + lane] = rec_n; nopen_rec[b0 + lane] = (uint8_t)rec_nopen;
      if (gated) open_rec[b0 + lane] = (uint8_t)rec_open;
    }
    const int done = min(p.n_blocks - b0, NSTEP); /* the trip's blocks: its last 64 samples are the next trip's carried ones */
    const float keep = x[done * BLOCK + lane];
    wg_sync<1>(); /* every lane has read the trip */
    x[lane] = keep;
  }
  w[NZ_HIST + lane] = __float_as_uint(x[lane]); /* the lane's own word: no fence needed */
  if (lane == 0) {
    w[NZ_KEY] = st.key; w[NZ_N] = __float_as_uint(st.N); w[NZ_OPEN] = (uint32_t)st.open; w[NZ_HANG] = (uint32_t)st.hang;
    if (gated) p.meter_words[(size_t)ch * MT_WORDS + MT_ANY] = __int_as_float(any);
  }
}

hipError_t rdsp_engine_noise_launch(const NoiseParams &p, hipStream_t s) {
  if (p.n_channels < 1 || p.n_blocks < 1) return hipSuccess;
  hipLaunchKernelGGL(rdsp_engine_noise_kernel, dim3((unsigned)((p.n_channels + NCH - 1) / NCH)), dim3(NW), 0, s, p);
  return hipGetLastError();
}
