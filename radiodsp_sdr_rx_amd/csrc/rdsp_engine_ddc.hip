/*
 * rdsp_engine_ddc.hip -- the decimating pass of rdsp_engine_update_sources for sources at D x 44 100 Hz, D > 1
 * (rdsp_engine_set_source_decimation, include/rdsp.h): every receiver's int16 row is its source row shifted to the
 * engine's IF, low-passed by a 16 D-tap FIR and decimated by D.  The definition and the order of the arithmetic are
 * rdsp_tune.h's (ddc_tap, ddc_mac, ddc_rot); D = 1 is rdsp_engine_tune.hip, which this file does not touch.
 *
 * Two kernels a call, in stream order:
 *   rdsp_engine_ddc_taps_kernel    g[ch][k] = h[k] e^{-j k dphi[ch]}, one lane a tap, vector stores;
 *   rdsp_engine_ddc_kernel         the filter bank (below);
 * after them the engine runs the finish kernel of both filter-bank passes (rdsp_engine_tune.hip): the last 15 D pairs of every
 * source row -> the engine's history, phases += n_out D dphi.
 *
 * The filter bank: a workgroup takes up to DDC_RPW receivers of ONE source that are neighbours in `order` and a tile of
 * 64 O outputs, O = 4, 2 or 1 by D (rdsp_engine_ddc_launch).  It stages the (64 O + 15) D pairs the tile needs in LDS once
 * for all of them, as floats, in polyphase order xs[r][n] = x[(m0 - 15 + n) D + r]: tap k = j D + p of output m0 + 64 o + lane
 * reads xs[D - 1 - p][64 o + lane + 15 - j], consecutive lanes consecutive 8-byte words whatever D is.  The pairs before the
 * call's first sample come from the history buffer.  The rows are read in the source's own format (a template parameter;
 * rdsp_tune.h's src_value is the one conversion, int16 pairs load as words, 8-bit pairs as 2-byte and float pairs as 8-byte
 * elements, coalesced along the source index all the same); the history holds packed words for int16 and float2 values for
 * the other formats, and the finish kernel writes whichever applies.  A lane is O outputs and a wave's DDC_C receivers are a register block
 * of DDC_C x O accumulator pairs: O ds_read_b64 and DDC_C taps feed 4 DDC_C O fmaf.  The taps are wave-uniform -- the
 * channel index goes through readfirstlane -- so they arrive by scalar loads from g, eight taps a load; with O > 1 the
 * compiler pairs two outputs of one tap into a v_pk_fma_f32, with O = 1 two receivers, which costs scalar moves to pair
 * their taps (3.1e8 scalar against 1.7e8 vector instructions per XCD at the ENGINE shape and D = 16, 5.0e7 at O = 4).  A
 * receiver slot past the workgroup's count computes its wave's first receiver again and stores nothing.
 *
 * Compiled with -ffp-contract=off: every fused operation is an fmaf.
 */
#include <hip/hip_runtime.h>

#include "rdsp_tune.h"

using namespace rdsp_tune;

namespace {

__global__ __launch_bounds__(DDC_THREADS) void rdsp_engine_ddc_taps_kernel(DdcParams p) {
  const uint32_t T = (uint32_t)(DDC_TAPS_PER_PHASE * p.D);
  const uint32_t i = blockIdx.x * DDC_THREADS + threadIdx.x;
  if (i >= (uint32_t)p.n_channels * T) return;
  const uint32_t ch = i / T, k = i - ch * T;
  p.g[i] = ddc_tap(p.tab, p.h[k], p.dphi[ch], k);
}

template <int F, int O> /* the format of the source rows; outputs per lane: a tile is 64 O outputs */
__global__ __launch_bounds__(DDC_THREADS) void rdsp_engine_ddc_kernel(DdcParams p) {
  constexpr int TILE = 64 * O, ROW = TILE + DDC_HIST_PER_PHASE;
  extern __shared__ float2 xs[]; /* [D][ROW] */
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int D = p.D, T = DDC_TAPS_PER_PHASE * D;
  const uint32_t n_tiles = p.n_out / TILE;
  const uint32_t wg = blockIdx.x / n_tiles, tile = blockIdx.x - wg * n_tiles;
  const int first = p.wg_first[wg], count = p.wg_count[wg];
  const uint32_t m0 = tile * TILE;

  /* stage: element e of the tile is x[(m0 - 15) D + e]; negative indices are the history's tail */
  {
    const int source = p.source_of[p.order[first]], keep = DDC_HIST_PER_PHASE * D;
    const void *row = src_at<F>(p.src, (size_t)source * p.src_stride);
    const uint32_t *hist = (const uint32_t *)p.hist + (size_t)source * (size_t)(keep * src_hist_words(F));
    const long long i0 = ((long long)m0 - DDC_HIST_PER_PHASE) * D;
    for (int e = tid; e < ROW * D; e += DDC_THREADS) {
      const int n = e / D, r = e - n * D;
      xs[r * ROW + n] = src_or_hist<F>(row, hist, i0 + e, keep);
    }
  }
  __syncthreads();
  if (wave * DDC_C >= count) return; /* a ragged last workgroup: this wave has no receiver */

  int ch[DDC_C];
  const float2 *g[DDC_C];
  float re[DDC_C][O], im[DDC_C][O];
#pragma unroll
  for (int c = 0; c < DDC_C; c++) {
    const int slot = wave * DDC_C + c < count ? wave * DDC_C + c : wave * DDC_C;
    ch[c] = __builtin_amdgcn_readfirstlane(p.order[first + slot]);
    g[c] = p.g + (size_t)ch[c] * (size_t)T;
#pragma unroll
    for (int o = 0; o < O; o++) re[c][o] = im[c][o] = 0.0f;
  }
  /* tap k = j D + p reads row D - 1 - p at lane + 15 - j */
  int ph = 0, at = (D - 1) * ROW + DDC_HIST_PER_PHASE;
  for (int k0 = 0; k0 < T; k0 += 8) {
#pragma unroll
    for (int u = 0; u < 8; u++) {
      float2 x[O];
#pragma unroll
      for (int o = 0; o < O; o++) x[o] = xs[at + 64 * o + lane];
#pragma unroll
      for (int c = 0; c < DDC_C; c++) {
        const float2 gk = g[c][k0 + u];
#pragma unroll
        for (int o = 0; o < O; o++) ddc_mac(re[c][o], im[c][o], gk, x[o].x, x[o].y);
      }
      ph++;
      at -= ROW;
      if (ph == D) { ph = 0; at += D * ROW - 1; }
    }
  }
#pragma unroll
  for (int c = 0; c < DDC_C; c++) {
    if (wave * DDC_C + c >= count) break;
    const uint32_t step = (uint32_t)D * p.dphi[ch[c]], ph0 = p.phase[ch[c]];
#pragma unroll
    for (int o = 0; o < O; o++) {
      const uint32_t m = m0 + (uint32_t)(64 * o + lane);
      p.dst[(size_t)ch[c] * p.dst_stride + m] = ddc_rot(re[c][o], im[c][o], tune_phasor(p.tab, tune_phase(ph0, step, m)));
    }
  }
}

constexpr size_t DDC_LDS_BUDGET = 163840 / 3;
size_t ddc_lds_bytes(int D, int O) { return (size_t)D * (size_t)(64 * O + DDC_HIST_PER_PHASE) * sizeof(float2); } /* at most 40 448 at O = 1 */

template <int F>
void ddc_launch(const DdcParams &p, int O, size_t grid, size_t lds, hipStream_t s) {
  if (O == 4) hipLaunchKernelGGL((rdsp_engine_ddc_kernel<F, 4>), dim3((unsigned)grid), dim3(DDC_THREADS), lds, s, p);
  else if (O == 2) hipLaunchKernelGGL((rdsp_engine_ddc_kernel<F, 2>), dim3((unsigned)grid), dim3(DDC_THREADS), lds, s, p);
  else hipLaunchKernelGGL((rdsp_engine_ddc_kernel<F, 1>), dim3((unsigned)grid), dim3(DDC_THREADS), lds, s, p);
}
}  // namespace

hipError_t rdsp_engine_ddc_launch(const DdcParams &p, hipStream_t s) {
  const size_t T = (size_t)(DDC_TAPS_PER_PHASE * p.D);
  const size_t n_g = (size_t)p.n_channels * T;
  /* outputs per lane: the most whose tile leaves room for three workgroups' LDS on a CU (measured: D = 24 runs faster at 4
   * than at 2, D = 30 and 40 faster at 2 than at 4 or 1, D = 56 and 64 no faster at 2 than at 1); 4 needs whole tiles of 256 */
  int O = 4;
  while (O > 1 && (ddc_lds_bytes(p.D, O) > DDC_LDS_BUDGET || p.n_out % (64u * O) != 0)) O >>= 1;
  const size_t lds = ddc_lds_bytes(p.D, O);
  const size_t grid = (size_t)p.n_wg * (p.n_out / (64u * O));
  if (grid > 0x7fffffffull) return hipErrorInvalidValue;
  return dispatch_format(p.format, [&](auto f) {
    hipLaunchKernelGGL(rdsp_engine_ddc_taps_kernel, dim3((unsigned)((n_g + DDC_THREADS - 1) / DDC_THREADS)), dim3(DDC_THREADS), 0, s, p);
    ddc_launch<decltype(f)::value>(p, O, grid, lds, s);
  });
}
