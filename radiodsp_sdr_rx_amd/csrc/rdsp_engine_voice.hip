/*
 * rdsp_engine_voice.hip -- rdsp_engine_t's voice-rate audio: the decimator that runs once per call behind the last group's
 * meter kernel, and the gather of rdsp_engine_pack_voice (include/rdsp.h has the definition, rdsp_voice.h the arithmetic).
 * Integers only; compiled with the engine's flags like the rest of the engine.
 *
 * rdsp_engine_voice_kernel<R>: one wave per channel, four channels a workgroup, no workgroup barrier (a wave past the last
 * channel leaves at once; the LDS of a wave is its own).  The wave walks its row in trips of 256 samples -- two blocks, one
 * 16-byte load a lane (four 4-byte loads when the caller's rows are not 16-byte aligned) -- and stages the left words in LDS as
 * words of two consecutive samples, by phase: R / 2 planes of 15 + 256 / R words, plane pp holding (x[R i + 2 pp], x[R i + 2 pp
 * + 1]) for the trip's output indices i and the 15 in front of them, so that lanes read consecutive words, not stride R.  Lane l
 * computes the trip's outputs l, l + 64 ... (4 / R of them).  The exact sum is taken in two halves, q = 256 hi + lo
 * (rdsp_voice.h): per word of two samples one 16-bit dot product with the word of the two hi parts and one with the word of the
 * lo parts, each into an int32 that cannot overflow; acc = 256 sum_hi + sum_lo in int64 is the definition's acc, whatever the
 * order.  The tap words are wave-uniform and come through the constant address space into scalar registers.  A trip's last 15
 * words of every plane move to the front for the next trip; the first trip's come from the channel's history, which the wave
 * read before it and renews behind the last trip from the row's last 60 words (a call is at least one block).  An odd count of
 * blocks ends in half a trip: the lanes past the row load nothing and store nothing.
 * rdsp_engine_voice_gather_kernel<R>: the pack's gather over blocks of 128 / R words out of the engine's voice rows, behind the
 * pack's own count and scan launches.  One wave per channel as there; per trip of 64 blocks the open ones leave their block
 * index at their rank in the wave's LDS, then 16 / R lanes copy a block with a 16-byte load and store each, 4 R blocks a step;
 * the first lane of a block writes the record.  Nothing at or behind `written` is written, a closed block is never read.
 */
#include <hip/hip_runtime.h>

#include "rdsp_engine_voice.h"
#include "rdsp_sync.h"

using namespace rdsp_eng;
using namespace rdsp_voice;

namespace {
constexpr int VW = 256, VCH = VW / 64; /* four waves, four channels */
constexpr int TRIP = 256;              /* samples a trip: four a lane */
constexpr int LEAD = TAPS_PER_PHASE - 1;

typedef const __attribute__((address_space(4))) int32_t *ConstTaps;
typedef short short2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int left_of(int32_t word) { return (int)(int16_t)(word & 0xFFFF); }
/* the left words of two {L, R} pairs, the earlier sample in the low half */
__device__ __forceinline__ int32_t left_pair(int32_t w0, int32_t w1) { return (w0 & 0xFFFF) | (int32_t)((uint32_t)w1 << 16); }
__device__ __forceinline__ int dot2(int32_t samples, int32_t taps, int acc) {
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(short2_t, samples), __builtin_bit_cast(short2_t, taps), acc, false);
}

template <int R>
__device__ __forceinline__ void voice_channel(const VoiceParams &p, int ch, int lane, int32_t *plane /* [R / 2][LEAD + TRIP / R] */) {
  constexpr int NP = R / 2, NOUT = TRIP / R, PL = LEAD + NOUT, OPL = NOUT / 64;
  const int32_t *row = p.lr + (size_t)ch * p.lr_stride;
  int32_t *hist = p.hist + (size_t)ch * VOICE_HIST;
  int16_t *y = p.rows + (size_t)ch * p.row_stride;
  ConstTaps t = (ConstTaps)(uintptr_t)p.tap_pairs;
  const int n = p.n_blocks * BLOCK;
  /* the newest 15 R words of the history, two a lane: pair jj of them is plane jj % NP, entry jj / NP */
  if (lane < LEAD * NP) {
    const int32_t *h = hist + VOICE_HIST - LEAD * R + 2 * lane;
    plane[(lane % NP) * PL + lane / NP] = left_pair(h[0], h[1]);
  }
  for (int s0 = 0; s0 < n; s0 += TRIP) {
    const int s = s0 + 4 * lane;
    int4 v = make_int4(0, 0, 0, 0);
    if (s < n) { /* whole lanes: n is a multiple of 128 */
      if (p.lr_vec) v = *(const int4 *)(row + s);
      else v = make_int4(row[s], row[s + 1], row[s + 2], row[s + 3]);
    }
    const int32_t w[2] = {left_pair(v.x, v.y), left_pair(v.z, v.w)};
#pragma unroll
    for (int c = 0; c < 2; c++) plane[(((4 * lane + 2 * c) % R) / 2) * PL + LEAD + (4 * lane + 2 * c) / R] = w[c];
    wg_sync<1>();
#pragma unroll
    for (int o = 0; o < OPL; o++) {
      const int i = lane + 64 * o;
      int sum_hi = 0, sum_lo = 0;
#pragma unroll
      for (int a = 0; a < TAPS_PER_PHASE; a++)
#pragma unroll
        for (int pp = 0; pp < NP; pp++) {
          const int32_t x = plane[pp * PL + LEAD + i - a];
          sum_hi = dot2(x, t[(a * NP + pp) * 2], sum_hi);
          sum_lo = dot2(x, t[(a * NP + pp) * 2 + 1], sum_lo);
        }
      const int m = s0 / R + i;
      if (m < n / R) y[m] = voice_round_sat(voice_acc_join(sum_hi, sum_lo));
    }
    int32_t keep = 0;
    if (lane < LEAD * NP) keep = plane[(lane / LEAD) * PL + NOUT + lane % LEAD];
    wg_sync<1>(); /* every lane has read the trip */
    if (lane < LEAD * NP) plane[(lane / LEAD) * PL + lane % LEAD] = keep;
  }
  if (lane < VOICE_HIST) hist[lane] = left_of(row[n - VOICE_HIST + lane]);
}
}  // namespace

template <int R>
__global__ __launch_bounds__(VW) void rdsp_engine_voice_kernel(const VoiceParams p) {
  __shared__ int32_t planes[VCH][(R / 2) * (LEAD + TRIP / R)];
  const int wave = (int)threadIdx.x >> 6;
  const int ch = (int)blockIdx.x * VCH + wave;
  if (ch >= p.n_channels) return;
  voice_channel<R>(p, ch, (int)threadIdx.x & 63, planes[wave]);
}

template <int R>
__global__ __launch_bounds__(VW) void rdsp_engine_voice_gather_kernel(const VoicePackParams p) {
  constexpr int LPB = 16 / R, BPS = 64 / LPB; /* lanes a block (16 bytes each), blocks a step */
  __shared__ int block_at[VCH][64];
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int ch = (int)blockIdx.x * VCH + wave;
  if (blockIdx.x == 0 && threadIdx.x == 0) p.counts[1] = min(p.counts[0], p.capacity); /* the scan ran with no capacity */
  if (ch >= p.n_channels) return;
  const int sub = lane / LPB, li = lane % LPB;
  const uint8_t *gate = p.open + (size_t)ch * p.rec_stride;
  const int4 *row = (const int4 *)(p.rows + (size_t)ch * p.row_stride);
  int4 *audio = (int4 *)p.audio;
  int *rank_to_block = block_at[wave];
  int at = p.offset[ch]; /* where the channel's next open block goes */
  for (int b0 = 0; b0 < p.n_blocks && at < p.capacity; b0 += 64) {
    const int b = b0 + lane;
    const unsigned long long m = __ballot(b < p.n_blocks && gate[b] != 0);
    const int open_here = __popcll(m), todo = min(open_here, p.capacity - at); /* wave-uniform */
    wg_sync<1>(); /* the trip in front has read its ranks */
    if ((m >> lane) & 1ull) rank_to_block[__popcll(m & ((1ull << lane) - 1ull))] = b;
    wg_sync<1>();
    for (int j0 = 0; j0 < todo; j0 += BPS) {
      const int j = j0 + sub;
      if (j < todo) {
        const int blk = rank_to_block[j];
        const size_t dst = (size_t)(at + j);
        audio[dst * LPB + li] = row[(size_t)blk * LPB + li];
        if (li == 0) p.records[dst] = make_int2(ch, blk);
      }
    }
    at += open_here;
  }
}

hipError_t rdsp_engine_voice_launch(const VoiceParams &p, hipStream_t s) {
  if (p.n_channels < 1 || p.n_blocks < 1) return hipSuccess;
  const dim3 grid((unsigned)((p.n_channels + VCH - 1) / VCH));
  if (p.R == 2) hipLaunchKernelGGL(rdsp_engine_voice_kernel<2>, grid, dim3(VW), 0, s, p);
  else if (p.R == 4) hipLaunchKernelGGL(rdsp_engine_voice_kernel<4>, grid, dim3(VW), 0, s, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}
hipError_t rdsp_engine_voice_gather_launch(const VoicePackParams &p, hipStream_t s) {
  if (p.n_channels < 1 || p.n_blocks < 1 || p.capacity < 1) return hipSuccess;
  const dim3 grid((unsigned)((p.n_channels + VCH - 1) / VCH));
  if (p.R == 2) hipLaunchKernelGGL(rdsp_engine_voice_gather_kernel<2>, grid, dim3(VW), 0, s, p);
  else if (p.R == 4) hipLaunchKernelGGL(rdsp_engine_voice_gather_kernel<4>, grid, dim3(VW), 0, s, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}
