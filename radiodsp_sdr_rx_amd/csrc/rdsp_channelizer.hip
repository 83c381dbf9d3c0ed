/*
 * rdsp_channelizer.hip -- rdsp_channelizer_t (include/rdsp.h): per source, a polyphase channelizer that splits the band once
 * into M overlapping sub-bands at D2 x 44 100 Hz, float2 rows that every engine reads as RDSP_SRC_F32 sources at the integer
 * rate D2.  The host-only half (rate, prototype, twiddles, placement) is rdsp_channelizer_host.cpp.
 *
 * Definition (include/rdsp.h has it in full): output instant i of a call has its newest source pair at n(i) and uses branch
 * r(i) of the prototype, the polyphase pass's schedule with P1 / Q1 = P / (Q D2); N = T + n(i) is that pair's index since the
 * reset.  Fold: v[q] = sum over the taps j with (N - j) mod M = q, ascending, of hb[r][j] x[n - j], one fmaf chain per
 * component.  DFT: sub-band k is sum_q twiddles[(k q) mod M]^* v[q], q ascending, four fmaf a term.
 *
 * The kernel: a workgroup of four waves takes one source and a tile of 64 output instants, a lane an instant.  It stages the
 * pairs the tile reads in LDS once, as values.  The chains of the fold are independent: chain m = (N - q) mod M takes the taps
 * m, m + M, m + 2 M ... in that order whatever q is, so wave w folds the chains m = w M / 4 ... (w + 1) M / 4 - 1 in registers with
 * static indices (its taps are M / 4 neighbours of a branch row, one vector load a lane) and only the store to vs[q][lane]
 * in LDS depends on the lane's N -- one bank per lane, whatever q.  After a barrier wave w reads all M v[q] of its lane into
 * registers and evaluates the sub-bands k = w M / 4 ... one after the other: k is wave-uniform, so row k of the [M][M] table of
 * twiddles[(k q) mod M] arrives by scalar loads, and a sub-band's 64 outputs leave as one 512-byte store.
 *
 * The finish kernel keeps the last Tb pairs of every source row as values; frac and T mod M advance on the host.
 * Compiled with -ffp-contract=off: every fused operation is an fmaf.
 */
#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "rdsp_channelizer.h"
#include "rdsp_dev.h"
#include "rdsp_host.h"

using namespace rdsp_tune;
using namespace rdsp_chan;

namespace {

/* pair i of the call's row, or for i < 0 of the Tb values kept from the calls before */
template <int F>
__device__ __forceinline__ float2 chan_pair(const void *row, const float2 *hist, long long i, int Tb) {
  return i >= 0 ? src_pair<F>(row, i) : hist[i + Tb];
}

template <int M, int F>
__global__ __launch_bounds__(THREADS) void rdsp_channelizer_kernel(Params p) {
  constexpr int MW = M / 4; /* chains of the fold, and sub-bands, per wave */
  static_assert(MW == 2 || MW % 4 == 0, "a wave's taps load as float2 or float4");
  extern __shared__ float2 lds[];
  float2 *vs = lds;            /* [M][TILE] */
  float2 *xs = lds + M * TILE; /* [xs_cap] */
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int src = blockIdx.y;
  const uint32_t i0 = blockIdx.x * TILE;
  const int Tb = p.Tb;

  /* stage: xs[e] = x[lo + e], lo the oldest pair the tile's first instant reads */
  const RateStep s0 = rate_step(p.frac, p.P1, p.Q1, i0), s1 = rate_step(p.frac, p.P1, p.Q1, i0 + (TILE - 1));
  const int lo = s0.n - (Tb - 1);
  {
    int cnt = s1.n - lo + 1; /* at most tile_pairs(Dc1) = xs_cap */
    if (cnt > p.xs_cap) cnt = p.xs_cap;
    const void *row = src_at<F>(p.src, (size_t)src * p.src_stride);
    const float2 *hist = p.hist + (size_t)src * (size_t)Tb;
    for (int e = tid; e < cnt; e += THREADS) xs[e] = chan_pair<F>(row, hist, (long long)lo + e, Tb);
  }
  __syncthreads();

  /* fold: this wave's MW chains of the lane's instant */
  {
    const RateStep st = rate_step(p.frac, p.P1, p.Q1, i0 + (uint32_t)lane);
    const float *hb = p.hb + (size_t)st.r * (size_t)Tb;
    const int at = st.n - lo; /* tap j reads xs[at - j]; at >= Tb - 1 */
    float wi[MW], wq[MW];
#pragma unroll
    for (int u = 0; u < MW; u++) wi[u] = wq[u] = 0.0f;
    for (int j0 = wave * MW; j0 < Tb; j0 += M) { /* Tb is a multiple of 16, j0 of MW: the MW taps lie inside the row */
      float h[MW];
      if constexpr (MW == 2) {
        const float2 t = *reinterpret_cast<const float2 *>(hb + j0);
        h[0] = t.x; h[1] = t.y;
      } else {
#pragma unroll
        for (int g = 0; g < MW / 4; g++) {
          const float4 t = reinterpret_cast<const float4 *>(hb + j0)[g];
          h[4 * g] = t.x; h[4 * g + 1] = t.y; h[4 * g + 2] = t.z; h[4 * g + 3] = t.w;
        }
      }
#pragma unroll
      for (int u = 0; u < MW; u++) {
        const float2 x = xs[at - j0 - u];
        wi[u] = fmaf(h[u], x.x, wi[u]);
        wq[u] = fmaf(h[u], x.y, wq[u]);
      }
    }
    const uint32_t N = p.tmod + (uint32_t)st.n;
#pragma unroll
    for (int u = 0; u < MW; u++) {
      const uint32_t q = (N - (uint32_t)(wave * MW + u)) & (uint32_t)(M - 1);
      vs[q * TILE + lane] = make_float2(wi[u], wq[u]);
    }
  }
  __syncthreads();

  /* DFT: this wave's MW sub-bands */
  float2 v[M];
#pragma unroll
  for (int q = 0; q < M; q++) v[q] = vs[q * TILE + lane];
  float2 *out = p.sub + ((size_t)src * M + (size_t)(wave * MW)) * p.sub_stride + i0 + lane;
  /* the table is read-only for the whole launch and the row is wave-uniform: through the constant address space its loads are
   * scalar, whatever the stores to p.sub between them may alias */
  typedef const __attribute__((address_space(4))) float2 *ConstRow;
  ConstRow tw = (ConstRow)(uintptr_t)(p.tw + (size_t)(wave * MW) * M);
#pragma unroll 1
  for (int kk = 0; kk < MW; kk++, tw += M, out += p.sub_stride) {
    float re = 0.0f, im = 0.0f;
#pragma unroll
    for (int q = 0; q < M; q++) {
      const float c = tw[q].x, s = tw[q].y;
      re = fmaf(c, v[q].x, re);
      re = fmaf(s, v[q].y, re);
      im = fmaf(c, v[q].y, im);
      im = fmaf(-s, v[q].x, im);
    }
    *out = make_float2(re, im);
  }
}

/* after the sub-bands, in their stream: the last Tb of the call's pairs (a call holds at least Tb) -> the history, as values */
template <int F>
__global__ __launch_bounds__(256) void rdsp_channelizer_finish_kernel(Params p) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  const int src = blockIdx.y;
  if (m >= p.Tb) return;
  const void *row = src_at<F>(p.src, (size_t)src * p.src_stride);
  p.hist[(size_t)src * (size_t)p.Tb + m] = src_pair<F>(row, (long long)p.pairs - p.Tb + m);
}

template <int M>
hipError_t chan_launch(int fmt, const Params &p, int n_sources, hipStream_t s) {
  const size_t lds = ((size_t)M * TILE + (size_t)p.xs_cap) * sizeof(float2);
  if (lds > 65536 || p.pairs < (uint32_t)p.Tb) return hipErrorInvalidValue;
  return dispatch_format(fmt, [&](auto f) {
    constexpr int F = decltype(f)::value;
    hipLaunchKernelGGL((rdsp_channelizer_kernel<M, F>), dim3(p.n_out / TILE, n_sources), dim3(THREADS), lds, s, p);
    hipLaunchKernelGGL((rdsp_channelizer_finish_kernel<F>), dim3((p.Tb + 255) / 256, n_sources), dim3(256), 0, s, p);
  });
}

}  // namespace

hipError_t rdsp_channelizer_launch(int M, int format, const Params &p, int n_sources, hipStream_t s) {
  switch (M) {
    case 8: return chan_launch<8>(format, p, n_sources, s);
    case 16: return chan_launch<16>(format, p, n_sources, s);
    case 32: return chan_launch<32>(format, p, n_sources, s);
    case 64: return chan_launch<64>(format, p, n_sources, s);
    default: return hipErrorInvalidValue;
  }
}

struct rdsp_channelizer {
  int n_sources, device, P, Q, M, D2, format, max_blocks;
  int P1, Q1, Tb;
  uint32_t frac = 0, tmod = 0; /* the schedule's remainder; T mod M, T the pairs consumed since the last reset */
  rdsp_dev::DevBuf<float2> d_hist, d_tw;
  rdsp_dev::DevBuf<float> d_hb;
};

namespace {
constexpr int CHAN_MAX_SOURCES = 4096, CHAN_MAX_BLOCKS = 4096;
uint32_t chan_n_out(const rdsp_channelizer_t *c, int n_blocks) { return (uint32_t)n_blocks * 128u * (uint32_t)c->D2; }
}  // namespace

extern "C" int rdsp_channelizer_create(int n_sources, int device, int P, int Q, int M, int D2, int format, int max_blocks_per_call,
                                       rdsp_channelizer_t **out) {
  int P1 = 0, Q1 = 0;
  if (!out || n_sources < 1 || n_sources > CHAN_MAX_SOURCES || format < 0 || format >= SRC_FORMATS || max_blocks_per_call < 1 ||
      max_blocks_per_call > CHAN_MAX_BLOCKS || !m_ok(M)) {
    rdsp_set_error("rdsp_channelizer_create: 1 ... %d sources, M 8, 16, 32 or 64, a format RDSP_SRC_*, max_blocks_per_call 1 ... %d",
                   CHAN_MAX_SOURCES, CHAN_MAX_BLOCKS);
    return RDSP_ERR_INVALID;
  }
  RC_TRY(rdsp_channelizer_rate(P, Q, D2, &P1, &Q1));
  (void)rate_reduce(P, Q); /* passed inside rdsp_channelizer_rate */
  if (!band_ok(P, Q, M, D2)) {
    rdsp_set_error("rdsp_channelizer_create: fs / (2 M) + 12000 <= 12000 D2 does not hold at 44100 x %d / %d Hz, M = %d, D2 = %d: a "
                   "station half a spacing from a sub-band centre would leave the prototype's flat band", P, Q, M, D2);
    return RDSP_ERR_INVALID;
  }
  RC_TRY(rdsp_dev::need_device());
  const int Tb = rate_tb(P1, Q1);
  std::vector<float> h((size_t)Tb * (size_t)Q1), hb((size_t)Tb * (size_t)Q1), tw((size_t)2 * M), tw2((size_t)2 * M * M);
  RC_TRY(rdsp_channelizer_taps(P, Q, D2, h.data()));
  RC_TRY(rdsp_channelizer_twiddles(M, tw.data()));
  for (int r = 0; r < Q1; r++)
    for (int j = 0; j < Tb; j++) hb[(size_t)r * Tb + j] = h[(size_t)j * Q1 + r];
  for (int k = 0; k < M; k++)
    for (int q = 0; q < M; q++) {
      const int m = (k * q) % M;
      tw2[2 * ((size_t)k * M + q)] = tw[2 * m];
      tw2[2 * ((size_t)k * M + q) + 1] = tw[2 * m + 1];
    }
  rdsp_channelizer_t *c = new rdsp_channelizer();
  c->n_sources = n_sources; c->device = device;
  c->P = P; c->Q = Q; c->M = M; c->D2 = D2;
  c->format = format; c->max_blocks = max_blocks_per_call;
  c->P1 = P1; c->Q1 = Q1; c->Tb = Tb;
  const bool ok = hipSetDevice(device) == hipSuccess && rdsp_dev::alloc_zero(c->d_hist, (size_t)n_sources * Tb) == hipSuccess &&
                  c->d_hb.alloc(hb.size()) == hipSuccess && c->d_tw.alloc((size_t)M * M) == hipSuccess &&
                  hipMemcpy(c->d_hb, hb.data(), hb.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(c->d_tw, tw2.data(), tw2.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    rdsp_set_error("rdsp_channelizer_create: device set-up failed");
    rdsp_channelizer_destroy(c);
    return RDSP_ERR_HIP;
  }
  *out = c;
  return RDSP_OK;
}
extern "C" void rdsp_channelizer_destroy(rdsp_channelizer_t *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  delete c;
}
extern "C" int rdsp_channelizer_sources(const rdsp_channelizer_t *c) { return c ? c->n_sources : 0; }
extern "C" int rdsp_channelizer_subbands(const rdsp_channelizer_t *c) { return c ? c->M : 0; }
extern "C" int rdsp_channelizer_decimation(const rdsp_channelizer_t *c) { return c ? c->D2 : 0; }
extern "C" int rdsp_channelizer_source_rate(const rdsp_channelizer_t *c, int *P, int *Q) {
  if (!c || !P || !Q) return RDSP_ERR_INVALID;
  *P = c->P; *Q = c->Q;
  return RDSP_OK;
}
extern "C" int rdsp_channelizer_format(const rdsp_channelizer_t *c) { return c ? c->format : -1; }
extern "C" int rdsp_channelizer_device(const rdsp_channelizer_t *c) { return c ? c->device : -1; }

extern "C" int rdsp_channelizer_reset(rdsp_channelizer_t *c, void *stream) {
  if (!c) {
    rdsp_set_error("rdsp_channelizer_reset: NULL object");
    return RDSP_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemsetAsync(c->d_hist, 0, (size_t)c->n_sources * (size_t)c->Tb * sizeof(float2), (hipStream_t)stream));
  c->frac = 0;
  c->tmod = 0;
  return RDSP_OK;
}

extern "C" size_t rdsp_channelizer_source_pairs(const rdsp_channelizer_t *c, int n_blocks) {
  if (!c || n_blocks < 0 || n_blocks > CHAN_MAX_BLOCKS) return 0;
  return (size_t)rate_pairs(c->frac, c->P1, c->Q1, chan_n_out(c, n_blocks));
}

extern "C" int rdsp_channelizer_update(rdsp_channelizer_t *c, const void *d_src, size_t src_stride, int n_blocks, float *d_sub,
                                       size_t sub_stride, void *stream) {
  if (!c) {
    rdsp_set_error("rdsp_channelizer_update: NULL object");
    return RDSP_ERR_INVALID;
  }
  if (n_blocks < 0 || n_blocks > c->max_blocks) {
    rdsp_set_error("rdsp_channelizer_update: %d blocks, the object was created for calls of at most %d", n_blocks, c->max_blocks);
    return RDSP_ERR_INVALID;
  }
  const uint32_t n_out = chan_n_out(c, n_blocks);
  const size_t pairs = (size_t)rate_pairs(c->frac, c->P1, c->Q1, n_out);
  if (src_stride < pairs || (pairs > 0 && !d_src) || ((uintptr_t)d_src % (uintptr_t)src_pair_bytes(c->format)) != 0) {
    rdsp_set_error("rdsp_channelizer_update: source rows aligned to one pair (%d bytes), src_stride at least "
                   "rdsp_channelizer_source_pairs = %zu", src_pair_bytes(c->format), pairs);
    return RDSP_ERR_INVALID;
  }
  if (sub_stride % 2 != 0 || sub_stride < (size_t)n_out || ((uintptr_t)d_sub & 15u) != 0 || (n_out > 0 && !d_sub)) {
    rdsp_set_error("rdsp_channelizer_update: d_sub 16-byte aligned, sub_stride even and at least n_blocks x 128 x D2 = %u pairs", n_out);
    return RDSP_ERR_INVALID;
  }
  if (n_blocks == 0) return RDSP_OK;
  HIP_TRY(hipSetDevice(c->device));
  Params p;
  memset(&p, 0, sizeof(p));
  p.src = d_src; p.src_stride = src_stride;
  p.hist = c->d_hist;
  p.hb = c->d_hb;
  p.tw = c->d_tw;
  p.sub = (float2 *)d_sub; p.sub_stride = sub_stride;
  p.P1 = c->P1; p.Q1 = c->Q1; p.Tb = c->Tb;
  p.xs_cap = tile_pairs(rate_dc(c->P1, c->Q1));
  p.frac = c->frac; p.tmod = c->tmod;
  p.n_out = n_out; p.pairs = (uint32_t)pairs;
  const hipError_t e = rdsp_channelizer_launch(c->M, c->format, p, c->n_sources, (hipStream_t)stream);
  if (e != hipSuccess) {
    rdsp_set_error("rdsp_channelizer_update: kernel launch failed: %s", hipGetErrorString(e));
    return RDSP_ERR_HIP;
  }
  c->frac = rate_frac_after(c->frac, c->P1, c->Q1, n_out);
  c->tmod = (uint32_t)((c->tmod + pairs) % (size_t)c->M);
  return RDSP_OK;
}
