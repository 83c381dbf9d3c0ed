/*
 * rdsp_engine_rate.hip -- the polyphase pass of rdsp_engine_update_sources for sources at 44 100 P / Q Hz, Q > 1
 * (rdsp_engine_set_source_rate, include/rdsp.h): every receiver's int16 row is its source row shifted to the engine's IF,
 * low-passed by branch r(i) of a 16 Dc Q-tap prototype and resampled by Q / P.  The definition, the schedule and the order
 * of the arithmetic are rdsp_tune.h's (rate_step, rate_u, ddc_mac, rate_phase, ddc_rot); Q = 1 is rdsp_engine_ddc.hip, which
 * this file does not touch.
 *
 * Two kernels a call, in stream order:
 *   rdsp_engine_rate_sched_kernel   sched[i] = {n(i), r(i)}, the 64-bit divisions of the schedule, once per output;
 *   rdsp_engine_rate_kernel         the filter bank (below);
 * after them the engine runs the finish kernel of both filter-bank passes (rdsp_engine_tune.hip): the last Tb pairs of every
 * source row -> the engine's history, phases += pairs dphi.
 *
 * The filter bank.  Consecutive outputs use different branches and their windows start Dc or Dc - 1 pairs apart, so a lane
 * cannot be an output as in the decimating pass.  What IS uniform is everything that does not depend on the receiver: the
 * products u[o][j] = hb[r(o)][j] x[n(o) - j].  So a lane is RATE_C = 2 RECEIVERS.  A workgroup of four waves takes up to 256
 * receivers of ONE source that are neighbours in `order` and a tile of 32 outputs: wave w has the receivers of half w & 1
 * and the 16 outputs of half w >> 1, 2 x 16 accumulator pairs a lane.  The taps go through LDS RATE_CHUNK = 128 at a time
 * (so its use does not grow with Dc: 34 816 bytes of products and the 16 384-byte phasor table, three workgroups a CU):
 * all threads stage the chunk's products as floats (the rows are read in the source's own format, a template parameter:
 * rdsp_tune.h's src_value; the history holds words for int16, float2 values otherwise), us[j][half][I / Q][16], coalesced along j in global memory, rows 68
 * words apart so that the writes of consecutive j spread over the banks; then per tap a wave reads its 32 floats by eight
 * 16-byte reads at ONE address for all lanes (a broadcast, no bank conflicts), each lane looks up its two receivers' phasors
 * at 0 - j dphi in the table in LDS (tune_phasor), and 128 fmaf follow.  The accumulators stay in registers through the
 * chunks, so each chain still runs over j ascending.  A lane whose receiver slot is past the workgroup's count computes the
 * workgroup's first receiver again and stores nothing; a wave without receivers only stages.
 *
 * Compiled with -ffp-contract=off: every fused operation is an fmaf.
 */
#include <hip/hip_runtime.h>

#include "rdsp_tune.h"

using namespace rdsp_tune;

namespace {

constexpr int RATE_PITCH = 4 * RATE_O + 4; /* floats from one tap's row to the next: 64 + 4 */

__global__ __launch_bounds__(RATE_THREADS) void rdsp_engine_rate_sched_kernel(RateParams p) {
  const uint32_t i = blockIdx.x * RATE_THREADS + threadIdx.x;
  if (i < p.n_out) p.sched[i] = rate_step(p.frac, p.P, p.Q, i);
}

template <int F> /* the format of the source rows (rdsp_tune.h, src_value) */
__global__ __launch_bounds__(RATE_THREADS) void rdsp_engine_rate_kernel(RateParams p) {
  __shared__ float4 tabs[TUNE_N];
  __shared__ __attribute__((aligned(16))) float us[RATE_CHUNK * RATE_PITCH];
  __shared__ RateStep steps[RATE_TILE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave & 1, wo = wave >> 1;
  const int Tb = rate_tb(p.P, p.Q), Dc = rate_dc(p.P, p.Q);
  const uint32_t n_tiles = p.n_out / RATE_TILE;
  const uint32_t wg = blockIdx.x / n_tiles, tile = blockIdx.x - wg * n_tiles;
  const int first = p.wg_first[wg], count = p.wg_count[wg];
  const uint32_t i0 = tile * RATE_TILE;
  const int source = p.source_of[p.order[first]];
  const void *row = src_at<F>(p.src, (size_t)source * p.src_stride);
  const uint32_t *hist = (const uint32_t *)p.hist + (size_t)source * (size_t)(Tb * src_hist_words(F));

  for (int k = tid; k < TUNE_N; k += RATE_THREADS) tabs[k] = p.tab[k];
  if (tid < RATE_TILE) steps[tid] = p.sched[i0 + tid];
  const bool active = wr * 64 * RATE_C < count; /* wave-uniform */

  uint32_t dphi[RATE_C], ph[RATE_C];
  int ch[RATE_C];
  bool live[RATE_C];
  float re[RATE_C][RATE_O], im[RATE_C][RATE_O];
#pragma unroll
  for (int c = 0; c < RATE_C; c++) {
    const int slot = (wr * RATE_C + c) * 64 + lane;
    live[c] = slot < count;
    ch[c] = p.order[first + (live[c] ? slot : 0)];
    dphi[c] = p.dphi[ch[c]];
    ph[c] = 0u;
#pragma unroll
    for (int o = 0; o < RATE_O; o++) re[c][o] = im[c][o] = 0.0f;
  }
  __syncthreads();

  for (int j0 = 0; j0 < Tb; j0 += RATE_CHUNK) {
    const int len = min(RATE_CHUNK, Tb - j0); /* a multiple of 16 */
    /* stage: element e is output e / len of the tile, tap j0 + e % len; x at negative indices is the history's tail */
    for (int e = tid; e < RATE_TILE * len; e += RATE_THREADS) {
      const int o = e / len, jj = e - o * len, j = j0 + jj;
      const RateStep s = steps[o];
      const int at = s.n - j; /* >= -(Tb - 1) */
      const float2 u = rate_u(p.hb[(size_t)s.r * (size_t)Tb + (size_t)j], src_or_hist<F>(row, hist, at, Tb));
      float *d = us + jj * RATE_PITCH + (o / RATE_O) * (2 * RATE_O) + (o % RATE_O);
      d[0] = u.x;
      d[RATE_O] = u.y;
    }
    __syncthreads();
    if (active) {
#pragma unroll 2
      for (int jj = 0; jj < len; jj++) {
        float2 e[RATE_C];
#pragma unroll
        for (int c = 0; c < RATE_C; c++) {
          e[c] = tune_phasor(tabs, ph[c]);
          ph[c] -= dphi[c];
        }
        const float4 *u4 = (const float4 *)(us + jj * RATE_PITCH + wo * (2 * RATE_O));
        float ui[RATE_O], uq[RATE_O];
#pragma unroll
        for (int o = 0; o < RATE_O; o += 4) {
          const float4 a = u4[o / 4], b = u4[(RATE_O + o) / 4];
          ui[o] = a.x; ui[o + 1] = a.y; ui[o + 2] = a.z; ui[o + 3] = a.w;
          uq[o] = b.x; uq[o + 1] = b.y; uq[o + 2] = b.z; uq[o + 3] = b.w;
        }
#pragma unroll
        for (int c = 0; c < RATE_C; c++)
#pragma unroll
          for (int o = 0; o < RATE_O; o++) ddc_mac(re[c][o], im[c][o], e[c], ui[o], uq[o]);
      }
    }
    __syncthreads(); /* the next chunk overwrites us */
  }
  if (!active) return;
#pragma unroll
  for (int c = 0; c < RATE_C; c++) {
    if (!live[c]) continue;
    const uint32_t ph0 = p.phase[ch[c]];
    uint4 *out = (uint4 *)(p.dst + (size_t)ch[c] * p.dst_stride + i0 + (uint32_t)(wo * RATE_O)); /* 64-byte aligned: rdsp_engine_rate_launch */
#pragma unroll
    for (int o = 0; o < RATE_O; o += 4) {
      uint32_t w[4];
#pragma unroll
      for (int k = 0; k < 4; k++)
        w[k] = ddc_rot(re[c][o + k], im[c][o + k], tune_phasor(tabs, rate_phase(ph0, dphi[c], steps[wo * RATE_O + o + k].n, Dc)));
      out[o / 4] = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
}

}  // namespace

hipError_t rdsp_engine_rate_launch(const RateParams &p, hipStream_t s) {
  /* the bank's vector stores: 16 outputs of a receiver are 64 bytes, whole in its row */
  if (p.n_out % RATE_TILE != 0 || p.dst_stride % 4 != 0 || ((uintptr_t)p.dst & 15) != 0 || p.pairs < (uint32_t)rate_tb(p.P, p.Q)) return hipErrorInvalidValue;
  const size_t grid = (size_t)p.n_wg * (p.n_out / RATE_TILE);
  if (grid > 0x7fffffffull) return hipErrorInvalidValue;
  return dispatch_format(p.format, [&](auto f) {
    hipLaunchKernelGGL(rdsp_engine_rate_sched_kernel, dim3((p.n_out + RATE_THREADS - 1) / RATE_THREADS), dim3(RATE_THREADS), 0, s, p);
    hipLaunchKernelGGL(rdsp_engine_rate_kernel<decltype(f)::value>, dim3((unsigned)grid), dim3(RATE_THREADS), 0, s, p);
  });
}
