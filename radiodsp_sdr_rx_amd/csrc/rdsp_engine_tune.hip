/*
 * rdsp_engine_tune.hip -- the tuning pass of rdsp_engine_update_sources (include/rdsp.h): every receiver's int16 row is
 * its source row times e^{+j phi[n]}, written to the engine's own [ch][max_blocks * 128] buffer, which the engine's
 * front kernels then read as they read a caller's rows.  The arithmetic is rdsp_tune.h's.
 *
 * A workgroup takes cpw receivers that are neighbours in `order` (receivers sorted by source, so a source row is read by
 * workgroups dispatched together and comes from the caches, not HBM), reads their phases and steps into LDS with the
 * phasor table, and streams each row in 16-byte words: four int16 pairs a lane (eight of 8-bit, two of float: the format of the
 * source rows is a template parameter, rdsp_tune.h's src_value the one conversion), phases in closed form ph0 + t dphi.  The phase
 * words are read before the one barrier and written after the last row, by the lanes that read them.
 *
 * The file also holds what the two filter-bank passes (rdsp_engine_ddc.hip, rdsp_engine_rate.hip) do after their banks, ONE
 * kernel for both: rdsp_engine_source_finish_kernel copies the last `keep` pairs of every source row into the engine's
 * history and advances every receiver's phase by pairs dphi.  It lives here because this is the pass file that belongs to no
 * rate: the host's front end (rdsp_engine_sources.hip) stays free of device code, and neither bank's file owns the other's tail.
 *
 * Compiled with -ffp-contract=off: every fused operation is an fmaf.
 */
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rdsp_tune.h"

using namespace rdsp_tune;

namespace {

template <int F> /* the format of the source rows (rdsp_tune.h, src_value) */
__global__ __launch_bounds__(TUNE_THREADS) void rdsp_engine_tune_kernel(TuneParams p) {
  __shared__ float4 tab[TUNE_N];
  __shared__ int ch_of[TUNE_MAX_CPW], src_of[TUNE_MAX_CPW];
  __shared__ uint32_t ph0_of[TUNE_MAX_CPW], dphi_of[TUNE_MAX_CPW];
  constexpr uint32_t NP = 16 / (F == SRC_F32 ? 8 : F == SRC_S16 ? 4 : 2); /* pairs in a lane's 16 bytes */
  const int tid = threadIdx.x;
  for (int k = tid; k < TUNE_N; k += TUNE_THREADS) tab[k] = p.tab[k];
  const int i0 = blockIdx.x * p.cpw;
  if (tid < p.cpw) {
    const int i = i0 + tid;
    const int ch = i < p.n_channels ? p.order[i] : -1;
    ch_of[tid] = ch;
    if (ch >= 0) { src_of[tid] = p.source_of[ch]; ph0_of[tid] = p.phase[ch]; dphi_of[tid] = p.dphi[ch]; }
  }
  __syncthreads();
  for (int k = 0; k < p.cpw; k++) {
    const int ch = ch_of[k];
    if (ch < 0) break;
    const uint4 *in = (const uint4 *)src_at<F>(p.src, (size_t)src_of[k] * p.src_stride);
    uint32_t *out = p.dst + (size_t)ch * p.dst_stride;
    const uint32_t ph0 = ph0_of[k], dphi = dphi_of[k];
    const uint32_t nv = p.n_samples / NP;
#pragma unroll 2
    for (uint32_t v = (uint32_t)tid; v < nv; v += TUNE_THREADS) {
      const uint4 w = in[v];
      const uint32_t ph = tune_phase(ph0, dphi, NP * v);
      if constexpr (F == SRC_S16) {
        uint4 r;
        r.x = tune_pair(w.x, tune_phasor(tab, ph));
        r.y = tune_pair(w.y, tune_phasor(tab, ph + dphi));
        r.z = tune_pair(w.z, tune_phasor(tab, ph + 2u * dphi));
        r.w = tune_pair(w.w, tune_phasor(tab, ph + 3u * dphi));
        ((uint4 *)out)[v] = r;
      } else if constexpr (F == SRC_F32) { /* two pairs: an 8-byte store */
        uint2 r;
        r.x = tune_pair(make_float2(src_value(F, w.x), src_value(F, w.y)), tune_phasor(tab, ph));
        r.y = tune_pair(make_float2(src_value(F, w.z), src_value(F, w.w)), tune_phasor(tab, ph + dphi));
        ((uint2 *)out)[v] = r;
      } else { /* eight pairs, two a word: two 16-byte stores */
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
        uint32_t r[8];
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) {
          const uint32_t b = ws[j >> 1] >> (16u * (j & 1u));
          r[j] = tune_pair(make_float2(src_value(F, b & 0xffu), src_value(F, (b >> 8) & 0xffu)), tune_phasor(tab, ph + j * dphi));
        }
        ((uint4 *)out)[2u * v] = make_uint4(r[0], r[1], r[2], r[3]);
        ((uint4 *)out)[2u * v + 1u] = make_uint4(r[4], r[5], r[6], r[7]);
      }
    }
  }
  if (tid < p.cpw && ch_of[tid] >= 0) p.phase[ch_of[tid]] = tune_phase(ph0_of[tid], dphi_of[tid], p.n_samples);
}

/* pairs >= keep: a call is at least 128 outputs, 128 D > 15 D pairs and 128 P / Q - 1 > 16 ceil(P / Q) (the launchers check) */
template <int F>
__global__ __launch_bounds__(TUNE_THREADS) void rdsp_engine_source_finish_kernel(SourceParams p, void *hist, uint32_t keep, uint32_t pairs, int n_sources) {
  const uint32_t i = blockIdx.x * TUNE_THREADS + threadIdx.x;
  if (i < (uint32_t)n_sources * keep) {
    const uint32_t s = i / keep, t = i - s * keep;
    const void *row = src_at<F>(p.src, (size_t)s * p.src_stride);
    if constexpr (F == SRC_S16) ((uint32_t *)hist)[i] = ((const uint32_t *)row)[(pairs - keep) + t];
    else ((float2 *)hist)[i] = src_pair<F>(row, (long long)(pairs - keep) + t);
  }
  if (i < (uint32_t)p.n_channels) p.phase[i] = tune_phase(p.phase[i], p.dphi[i], pairs);
}

}  // namespace

hipError_t rdsp_engine_tune_launch(const TuneParams &p, hipStream_t s) {
  const unsigned grid = (unsigned)((p.n_channels + p.cpw - 1) / p.cpw);
  return dispatch_format(p.format, [&](auto f) {
    hipLaunchKernelGGL(rdsp_engine_tune_kernel<decltype(f)::value>, dim3(grid), dim3(TUNE_THREADS), 0, s, p);
  });
}

hipError_t rdsp_engine_source_finish_launch(const SourceParams &p, void *hist, uint32_t keep, uint32_t pairs, int n_sources, hipStream_t s) {
  if (keep == 0 || pairs < keep || !hist) return hipErrorInvalidValue;
  const size_t n = std::max((size_t)n_sources * keep, (size_t)p.n_channels);
  return dispatch_format(p.format, [&](auto f) {
    hipLaunchKernelGGL(rdsp_engine_source_finish_kernel<decltype(f)::value>, dim3((unsigned)((n + TUNE_THREADS - 1) / TUNE_THREADS)), dim3(TUNE_THREADS), 0, s,
                       p, hist, keep, pairs, n_sources);
  });
}
