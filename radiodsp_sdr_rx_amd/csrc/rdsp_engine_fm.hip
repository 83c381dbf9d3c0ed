/*
 * rdsp_engine_fm.hip -- rdsp_engine_t's narrow-band FM detector: the kernel an NFM group launches where the other modes launch the
 * front and Hilbert kernels (include/rdsp.h has the definition, rdsp_fm.h the arithmetic).  It reads the group's int16 IQ rows
 * once (and a row's last 47 words a second time, for the state: 188 bytes a channel and call) and writes two float rows once:
 * y into the engine's demodulated rows, which the tail kernel then runs on unchanged, and the level rows, which the group's
 * meter is handed in their place.  Compiled with the engine's flags like the rest of it.
 *
 * rdsp_engine_fm_kernel<W, DE>: one wave per channel, four channels a workgroup, no workgroup barrier (a wave past the last
 * channel leaves at once; the LDS of a wave is its own).  The wave walks its row in trips of 256 samples -- one 16-byte load of
 * four pair words a lane (four 4-byte loads when the caller's rows are not 16-byte aligned) -- and stages I and Q as floats in
 * two LDS planes: the trip's sample s at word 48 + s, the 47 carried ones at words 1 ... 47, so that lane l's window of T + 3
 * values ends on a 16-byte boundary and is read as whole float4, sixteen taps' worth (five float4 a plane) at a time.  The taps
 * are wave-uniform and come through the constant address space into scalar registers.  Lane l runs the chains of samples 4 l
 * ... 4 l + 3 (k ascending, as the definition has them: four independent chains a component, which the compiler pairs into packed
 * fused multiply-adds); z[n - 1] of its first sample is lane l - 1's last z -- the same arithmetic, so the
 * same bits -- and lane 0's the wave's carry.  Then lvl, d and u a sample, stored as float4.  The one-pole de-emphasis is serial
 * in time: u goes through LDS, lane 0 walks the trip's valid samples (two dependent operations each) and every lane stores its
 * four y.  While one wave walks, the other three of its SIMD run their chains.  A trip's last 47 words of each plane move to the
 * front for the next trip; the first trip's come from the channel's state, which the wave renews behind the last trip from the
 * row's last 47 words (a call is at least one block).  An odd count of blocks ends in half a trip: the lanes past the row load
 * nothing and store nothing, and the carry is taken from the lane of the row's last sample.
 */
#include <hip/hip_runtime.h>

#include "rdsp_engine_fm.h"
#include "rdsp_sync.h"

using namespace rdsp_eng;
using namespace rdsp_fm;

namespace {
constexpr int FW = 256, FCH = FW / 64; /* four waves, four channels */
constexpr int TRIP = 256;              /* samples a trip: four a lane */
constexpr int LEAD = 48;               /* words in front of a trip's first sample in a plane; word 0 is never read */
constexpr int PLANE4 = (LEAD + TRIP) / 4;

typedef const __attribute__((address_space(4))) float *ConstTaps;

__device__ __forceinline__ float wave_value(float v, int lane) { return __shfl(v, lane); }

template <int W, bool DE>
__device__ __forceinline__ void fm_channel(const FmParams &p, int ch, int lane, float4 *pi4, float4 *pq4, float4 *u4) {
  constexpr int T = TAPS_PER_W * W;
  constexpr int CHUNK = 16, CHUNK4 = CHUNK / 4 + 1; /* a chunk's CHUNK + 3 words begin one word behind a 16-byte boundary: five float4 */
  const int32_t *row = p.iq + (size_t)ch * p.in_stride;
  uint32_t *state = p.state + (size_t)ch * FM_STATE_WORDS;
  float *ya = p.audio + (size_t)ch * p.audio_stride, *lv = p.level + (size_t)ch * p.level_stride;
  float *pi = (float *)pi4, *pq = (float *)pq4;
  ConstTaps t = (ConstTaps)(uintptr_t)p.taps;
  const int n = p.n_blocks * BLOCK;
  const bool fresh = p.reset != 0;
  if (lane < FM_HIST) {
    const uint32_t w = fresh ? 0u : state[lane];
    pi[1 + lane] = fm_i_of(w);
    pq[1 + lane] = fm_q_of(w);
  }
  float carry_i = fresh ? 0.0f : __uint_as_float(state[FM_ST_Z]), carry_q = fresh ? 0.0f : __uint_as_float(state[FM_ST_Z + 1]);
  float y1 = fresh ? 0.0f : __uint_as_float(state[FM_ST_Y]);
  for (int s0 = 0; s0 < n; s0 += TRIP) {
    const int s = s0 + 4 * lane;
    const int valid4 = min(n - s0, TRIP) / 4; /* lanes with samples: n is a multiple of 128 */
    int4 v = make_int4(0, 0, 0, 0);
    if (s < n) { /* whole lanes */
      if (p.in_vec) v = *(const int4 *)(row + s);
      else v = make_int4(row[s], row[s + 1], row[s + 2], row[s + 3]);
    }
    pi4[LEAD / 4 + lane] = make_float4(fm_i_of((uint32_t)v.x), fm_i_of((uint32_t)v.y), fm_i_of((uint32_t)v.z), fm_i_of((uint32_t)v.w));
    pq4[LEAD / 4 + lane] = make_float4(fm_q_of((uint32_t)v.x), fm_q_of((uint32_t)v.y), fm_q_of((uint32_t)v.z), fm_q_of((uint32_t)v.w));
    wg_sync<1>();
    float z[2][4] = {{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}};
    /* sixteen taps at a time, a loop that stays one: the four samples of taps k0 ... k0 + 15 read 19 words, which lie in five
     * float4 from the plane's word 4 (lane + f0) on, f0 = (32 - k0) / 4; sample j's x[n - k] is word 16 + j - (k - k0) of them.
     * The window of all T taps at once would be 2 (T + 4) registers, and 144 VGPRs at W = 3 */
#pragma unroll 1
    for (int k0 = 0; k0 < T; k0 += CHUNK) {
      const int f0 = (LEAD - CHUNK - k0) / 4;
      float w[2][4 * CHUNK4];
#pragma unroll
      for (int c = 0; c < 2; c++)
#pragma unroll
        for (int f = 0; f < CHUNK4; f++) {
          const float4 q = (c == 0 ? pi4 : pq4)[lane + f0 + f];
          w[c][4 * f] = q.x; w[c][4 * f + 1] = q.y; w[c][4 * f + 2] = q.z; w[c][4 * f + 3] = q.w;
        }
#pragma unroll
      for (int kk = 0; kk < CHUNK; kk++) {
        const float h = t[k0 + kk];
#pragma unroll
        for (int j = 0; j < 4; j++) fm_mac(z[0][j], z[1][j], h, w[0][CHUNK + j - kk], w[1][CHUNK + j - kk]);
      }
    }
    float prev_i = __shfl_up(z[0][3], 1), prev_q = __shfl_up(z[1][3], 1);
    if (lane == 0) { prev_i = carry_i; prev_q = carry_q; }
    carry_i = wave_value(z[0][3], valid4 - 1);
    carry_q = wave_value(z[1][3], valid4 - 1);
    float l[4], u[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      l[j] = fm_level(z[0][j], z[1][j]);
      u[j] = fm_detect(z[0][j], z[1][j], j == 0 ? prev_i : z[0][j - 1], j == 0 ? prev_q : z[1][j - 1], p.k);
    }
    if (s < n) *(float4 *)(lv + s) = make_float4(l[0], l[1], l[2], l[3]);
    if constexpr (DE) {
      u4[lane] = make_float4(u[0], u[1], u[2], u[3]);
      wg_sync<1>();
      if (lane == 0) {
        const float a = p.a;
#pragma unroll 8 /* valid4 is 32 or 64: eight reads in flight in front of the chain, not one LDS round trip every four samples */
        for (int i = 0; i < valid4; i++) {
          float4 q = u4[i];
          q.x = y1 = fm_deemph(a, q.x, y1);
          q.y = y1 = fm_deemph(a, q.y, y1);
          q.z = y1 = fm_deemph(a, q.z, y1);
          q.w = y1 = fm_deemph(a, q.w, y1);
          u4[i] = q;
        }
      }
      wg_sync<1>();
      if (s < n) *(float4 *)(ya + s) = u4[lane];
    } else {
      if (s < n) *(float4 *)(ya + s) = make_float4(u[0], u[1], u[2], u[3]);
      y1 = wave_value(u[3], valid4 - 1);
    }
    float keep_i = 0.0f, keep_q = 0.0f;
    if (lane < FM_HIST) { keep_i = pi[TRIP + 1 + lane]; keep_q = pq[TRIP + 1 + lane]; }
    wg_sync<1>(); /* every lane has read the trip */
    if (lane < FM_HIST) { pi[1 + lane] = keep_i; pq[1 + lane] = keep_q; }
  }
  y1 = wave_value(y1, 0);
  if (lane < FM_HIST) state[lane] = (uint32_t)row[n - FM_HIST + lane];
  else if (lane == FM_ST_Z) state[lane] = __float_as_uint(carry_i);
  else if (lane == FM_ST_Z + 1) state[lane] = __float_as_uint(carry_q);
  else if (lane == FM_ST_Y) state[lane] = __float_as_uint(y1);
}
}  // namespace

template <int W, bool DE>
__global__ __launch_bounds__(FW) void rdsp_engine_fm_kernel(const FmParams p) {
  __shared__ float4 plane_i[FCH][PLANE4], plane_q[FCH][PLANE4], row_u[FCH][DE ? TRIP / 4 : 1];
  const int wave = (int)threadIdx.x >> 6;
  const int ch = (int)blockIdx.x * FCH + wave;
  if (ch >= p.n_channels) return;
  fm_channel<W, DE>(p, ch, (int)threadIdx.x & 63, plane_i[wave], plane_q[wave], row_u[wave]);
}

hipError_t rdsp_engine_fm_launch(const FmParams &p, hipStream_t s) {
  if (p.n_channels < 1 || p.n_blocks < 1) return hipSuccess;
  const dim3 grid((unsigned)((p.n_channels + FCH - 1) / FCH));
  if (p.W == 2 && p.deemph) hipLaunchKernelGGL((rdsp_engine_fm_kernel<2, true>), grid, dim3(FW), 0, s, p);
  else if (p.W == 2) hipLaunchKernelGGL((rdsp_engine_fm_kernel<2, false>), grid, dim3(FW), 0, s, p);
  else if (p.W == 3 && p.deemph) hipLaunchKernelGGL((rdsp_engine_fm_kernel<3, true>), grid, dim3(FW), 0, s, p);
  else if (p.W == 3) hipLaunchKernelGGL((rdsp_engine_fm_kernel<3, false>), grid, dim3(FW), 0, s, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}
