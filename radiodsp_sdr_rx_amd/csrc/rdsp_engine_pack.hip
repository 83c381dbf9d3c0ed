/*
 * rdsp_engine_pack.hip -- rdsp_engine_pack_active's kernels: the blocks of the last call whose gate was open, gathered into
 * dense mono blocks with a {channel, block} record each, channel ascending, then block ascending (include/rdsp.h has the
 * definition).  Integers only; compiled with the engine's flags like the rest of the engine.  Three launches a call, no
 * atomics, nothing that waits on another workgroup:
 *
 * rdsp_engine_pack_count_kernel: one wave per channel, four channels a workgroup, no LDS, no barrier (a wave past the last
 * channel leaves at once).  The wave reads the channel's gate records 64 blocks a trip; a ballot's population count is the
 * trip's count of open blocks; lane 0 writes the channel's sum into offset[ch].
 * rdsp_engine_pack_scan_kernel: one workgroup walks the channels in ascending chunks of 1024, as rdsp_engine_active_kernel
 * does: a wave scan inside a wave, the waves' totals added in wave order through LDS, the chunks in chunk order.  offset[ch]
 * becomes the index of the channel's first packed block; the total is `needed`, min(needed, capacity) is `written`.
 * rdsp_engine_pack_gather_kernel: the count kernel's shape.  Per trip of 64 blocks the ballot of the open ones is walked from
 * its lowest bit, eight blocks a step: a half-wave holds one block, lane l of 32 loads the pairs 4 l ... 4 l + 3 with one
 * 16-byte load (four 4-byte loads when the caller's rows are not 16-byte aligned), four blocks a half-wave are loaded before
 * the first is stored (a half-wave whose slot of the step is empty loads the step's first block again, so no branch stands
 * between the loads), and the four left words leave with one 8-byte store; lane 0 of the half-wave writes the record.  The
 * blocks of a channel land at consecutive indices, so the capacity only shortens the trip's count (wave-uniform): nothing at
 * or behind `written` is written, and a closed block is never read.
 */
#include <hip/hip_runtime.h>

#include "rdsp_engine_pack.h"

using namespace rdsp_eng;

namespace {
constexpr int PBLOCK = 128;            /* samples a block */
constexpr int PW = 256, PCH = PW / 64; /* the count's and the gather's workgroup: four waves, four channels */
constexpr int PSTEP = 8;               /* blocks in flight per wave */
constexpr int SW = 1024;               /* the scan's workgroup */

/* which of a trip's 64 blocks are open: the same value in every lane */
__device__ __forceinline__ unsigned long long open_mask(const uint8_t *gate, int b0, int n_blocks, int lane) {
  const int b = b0 + lane;
  return __ballot(b < n_blocks && gate[b] != 0);
}
/* the left words of four {L, R} pairs */
__device__ __forceinline__ int2 left_words(int4 v) {
  return make_int2((v.x & 0xFFFF) | (int)((unsigned)v.y << 16), (v.z & 0xFFFF) | (int)((unsigned)v.w << 16));
}
}  // namespace

__global__ __launch_bounds__(PW) void rdsp_engine_pack_count_kernel(const PackParams p) {
  const int lane = (int)threadIdx.x & 63;
  const int ch = (int)blockIdx.x * PCH + ((int)threadIdx.x >> 6);
  if (ch >= p.n_channels) return;
  const uint8_t *gate = p.open + (size_t)ch * p.rec_stride;
  int n = 0;
  for (int b0 = 0; b0 < p.n_blocks; b0 += 64) n += __popcll(open_mask(gate, b0, p.n_blocks, lane));
  if (lane == 0) p.offset[ch] = n;
}

__global__ __launch_bounds__(SW) void rdsp_engine_pack_scan_kernel(const PackParams p) {
  __shared__ int wave_count[SW / 64];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int base = 0;
  for (int c0 = 0; c0 < p.n_channels; c0 += SW) { /* the same trips for every thread */
    const int c = c0 + tid;
    const int n = c < p.n_channels ? p.offset[c] : 0;
    int upto = n; /* the counts of the wave's lanes 0 ... lane */
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(upto, d);
      if (lane >= d) upto += t;
    }
    if (lane == 63) wave_count[wave] = upto;
    __syncthreads();
    int before = base, total = 0;
    for (int k = 0; k < SW / 64; k++) {
      if (k < wave) before += wave_count[k];
      total += wave_count[k];
    }
    if (c < p.n_channels) p.offset[c] = before + upto - n;
    base += total;
    __syncthreads(); /* wave_count is written again */
  }
  if (tid == 0) { p.counts[0] = base; p.counts[1] = min(base, p.capacity); }
}

/* VEC: the rows of p.lr are 16-byte aligned */
template <bool VEC>
__device__ __forceinline__ void gather_channel(const PackParams &p, int ch, int lane) {
  const int half = lane >> 5, l32 = lane & 31;
  const uint8_t *gate = p.open + (size_t)ch * p.rec_stride;
  const int32_t *row = p.lr + (size_t)ch * p.lr_stride + 4 * l32;
  int2 *audio = (int2 *)p.audio + l32;
  int at = p.offset[ch]; /* where the channel's next open block goes */
  for (int b0 = 0; b0 < p.n_blocks && at < p.capacity; b0 += 64) {
    unsigned long long m = open_mask(gate, b0, p.n_blocks, lane);
    const int open_here = __popcll(m), todo = min(open_here, p.capacity - at); /* wave-uniform */
    for (int j0 = 0; j0 < todo; j0 += PSTEP) {
      int4 v[PSTEP / 2];
      int blk[PSTEP / 2];
      const int first = __ffsll(m) - 1; /* open, and inside the capacity: what a half-wave without a block of its own loads again */
#pragma unroll
      for (int k = 0; k < PSTEP / 2; k++) { /* the mask's next two open blocks: the lower for lanes 0 ... 31 */
        const int lo = __ffsll(m) - 1;
        m &= m - 1ull;
        const int hi = __ffsll(m) - 1;
        m &= m - 1ull;
        blk[k] = b0 + (j0 + 2 * k + half < todo ? (half ? hi : lo) : first);
        const int32_t *src = row + (size_t)blk[k] * PBLOCK; /* no branch around the loads: all of a step's are issued before its first store */
        if (VEC) v[k] = *(const int4 *)src;
        else v[k] = make_int4(src[0], src[1], src[2], src[3]);
      }
#pragma unroll
      for (int k = 0; k < PSTEP / 2; k++) {
        if (j0 + 2 * k + half < todo) {
          const size_t dst = (size_t)(at + j0 + 2 * k + half);
          audio[dst * (PBLOCK / 4)] = left_words(v[k]);
          if (l32 == 0) p.records[dst] = make_int2(ch, blk[k]);
        }
      }
    }
    at += open_here;
  }
}

__global__ __launch_bounds__(PW) void rdsp_engine_pack_gather_kernel(const PackParams p) {
  const int ch = (int)blockIdx.x * PCH + ((int)threadIdx.x >> 6);
  if (ch >= p.n_channels) return;
  if (p.lr_vec) gather_channel<true>(p, ch, (int)threadIdx.x & 63);
  else gather_channel<false>(p, ch, (int)threadIdx.x & 63);
}

hipError_t rdsp_engine_pack_launch(const PackParams &p, hipStream_t s) {
  const dim3 per_channel((unsigned)((p.n_channels + PCH - 1) / PCH));
  hipLaunchKernelGGL(rdsp_engine_pack_count_kernel, per_channel, dim3(PW), 0, s, p);
  hipLaunchKernelGGL(rdsp_engine_pack_scan_kernel, dim3(1), dim3(SW), 0, s, p);
  if (p.capacity > 0) hipLaunchKernelGGL(rdsp_engine_pack_gather_kernel, per_channel, dim3(PW), 0, s, p);
  return hipGetLastError();
}
