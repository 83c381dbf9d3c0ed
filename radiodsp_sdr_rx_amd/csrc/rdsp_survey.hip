/*
 * rdsp_survey.hip -- rdsp_survey_t (include/rdsp.h): Welch-averaged power spectra of shared IQ source rows, the rows of
 * rdsp_engine_update_source_samples in their own format, as float rows on the device.  The host-only half (window, schedule,
 * axis, station finder) is rdsp_survey_host.c.
 *
 * Definition (include/rdsp.h has it in full): frame f covers pairs [f H, f H + N) of a source since the last reset, H = N / 2;
 * x_f[n] = w[n] v[n] (one rounded product per component), X_f the forward N-point transform, p_f[k] = |X_f[k]|^2; row r sums
 * the frames r navg ... r navg + navg - 1 in ascending order from 0 and scales by 1 / navg; bin k leaves at index
 * (k + N / 2) mod N.
 *
 * One workgroup per (source, row): N / 16 threads (one wave at 1024, four at 4096), FftPlan<N, 16> of rdsp_fft.h with the
 * product-chain twiddles.  Thread t holds pairs t + j NT (j < 16) of a frame, which is what the first pass wants and is
 * coalesced along t; the upper half of a frame is the lower half of the next (H = 8 NT), so the raw values stay in
 * registers and a frame loads eight new ones, issued before the passes of the frame before.  The powers are summed in
 * 16 registers at the transform's digit-reversed positions; after the row's last frame they go through LDS once and leave in
 * natural, shifted order as 16-byte stores.
 *
 * What makes the bits independent of the call split: a frame's arithmetic is a function of its N values (pairs before the
 * call come from a history of float2 VALUES), and the trailing, incomplete row of a call leaves its sum so far in a per-source
 * partial accumulator from which the first row of the next call continues -- the same adds in the same order.  The first
 * row's workgroup reads the partial sums while the last one's writes them, and the finish kernel moves pairs inside the
 * history: both buffers exist twice and a call reads one copy and writes the other.
 */
#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "rdsp_dev.h"
#include "rdsp_fft.h"
#include "rdsp_host.h"
#include "rdsp_sync.h"
#include "rdsp_tune.h"

using namespace rdsp;
using namespace rdsp_tune;

struct RdspSurveyParams {
  const void *src; size_t src_stride;  /* [source][pairs] in the object's format, the stride in pairs */
  const float2 *hist_in;               /* [source][N]: the hist_len pairs before the call, as values */
  float2 *hist_out;                    /* [source][N]: written by the finish kernel */
  const float *part_in;                /* [source][N]: the sum so far of the row the call's first frame belongs to */
  float *part_out;                     /* [source][N]: the same of the call's trailing row */
  const float *window;                 /* [N] */
  float *rows; size_t rows_stride;     /* [source][row][N], floats between sources */
  long long first;                     /* local index (pair 0 = the call's first) of the first pair of frame f0: -hist_len */
  int hist_len;
  int lead;                            /* f0 mod navg: frames the first row already has in part_in */
  int n_frames;                        /* frames the call completes */
  int navg;
  int keep; long long keep_from;       /* the finish kernel keeps `keep` pairs from local index keep_from on */
};

namespace {

constexpr int SURVEY_P = 16;

/* pair i of the call's row, or for i < 0 of the hist_len values kept from the calls before */
template <int F>
__device__ __forceinline__ float2 survey_pair(const void *row, const float2 *hist, long long i, int hist_len) {
  return i >= 0 ? src_pair<F>(row, i) : hist[i + hist_len];
}

/* acc + |x|^2, the power first: three rounded operations and a fused one, never contracted across the sum */
__device__ __forceinline__ float survey_add_power(float acc, float2 x) {
#pragma clang fp contract(off)
  const float p = fmaf(x.x, x.x, x.y * x.y);
  return acc + p;
}

template <int N, int F>
__global__ void __launch_bounds__(N / SURVEY_P) rdsp_survey_kernel(RdspSurveyParams p) {
  constexpr int P = SURVEY_P;
  using PL = FftPlan<N, P>;
  constexpr int NT = PL::NT, NW = NT / 64, H = N / 2;
  static_assert(NT == 64 || NT == 256, "one wave or four");
  static_assert(H == (P / 2) * NT, "the upper half of a thread's points is the lower half of the next frame's");
  static_assert(PL::WB * sizeof(float2) >= N * sizeof(float), "the row fits the work buffer");
  __shared__ __attribute__((aligned(16))) float2 wb[PL::WB];

  const int t = threadIdx.x;
  const int src = blockIdx.y;
  const int unit = blockIdx.x; /* row of the call; the one behind the last complete row is the trailing, partial one */
  /* frames of the call (0 = f0) this row takes: [g0, g1) */
  const long long rb = (long long)unit * p.navg - p.lead;
  const int g0 = rb < 0 ? 0 : (int)rb;
  const bool complete = rb + p.navg <= (long long)p.n_frames;
  const int g1 = complete ? (int)(rb + p.navg) : p.n_frames;

  const void *row = src_at<F>(p.src, (size_t)src * p.src_stride);
  const float2 *hist = p.hist_in + (size_t)src * N;

  Twiddles<N, P, true> tw;
  LdsBases<N, P, false> lb;
  tw.init(t);
  make_lds_bases<N, P, false>(t, lb);
  float w[P];
#pragma unroll
  for (int j = 0; j < P; j++) w[j] = p.window[t + j * NT];

  float acc[P];
  if (rb < 0) { /* the call's first row continues a row of the calls before */
    const float *pi = p.part_in + (size_t)src * N;
#pragma unroll
    for (int e = 0; e < P; e++) acc[e] = pi[e * NT + t];
  } else {
#pragma unroll
    for (int e = 0; e < P; e++) acc[e] = 0.0f;
  }

  float2 raw[P];
  {
    const long long i0 = p.first + (long long)g0 * H + t;
#pragma unroll
    for (int j = 0; j < P; j++) raw[j] = survey_pair<F>(row, hist, i0 + j * NT, p.hist_len);
  }
  auto sync = []() { wg_sync<NW>(); };
#pragma unroll 1
  for (int g = g0; g < g1; g++) {
    float2 v[P];
#pragma unroll
    for (int j = 0; j < P; j++) v[j] = make_float2(w[j] * raw[j].x, w[j] * raw[j].y);
#pragma unroll
    for (int j = 0; j < P / 2; j++) raw[j] = raw[j + P / 2];
    if (g + 1 < g1) { /* the next frame's new half lands behind the passes */
      const long long i0 = p.first + (long long)(g + 1) * H + H + t;
#pragma unroll
      for (int j = 0; j < P / 2; j++) raw[j + P / 2] = survey_pair<F>(row, hist, i0 + j * NT, p.hist_len);
    }
    {
      float2 twp[P - 1];
      tw.template get<0>(twp);
      fwd_pass0_store<N, P>(lb, v, wb, twp);
    }
    wg_sync<NW>();
    fwd_mid_all<N, P, 1, PL::NP - 1, false>(lb, wb, tw, sync);
    fwd_pass_last<N, P>(lb, v, wb);
    wg_sync<NW>(); /* wb is free again: the next frame, or the row below */
#pragma unroll
    for (int e = 0; e < P; e++) acc[e] = survey_add_power(acc[e], v[e]);
  }

  if (!complete) {
    float *po = p.part_out + (size_t)src * N;
#pragma unroll
    for (int e = 0; e < P; e++) po[e * NT + t] = acc[e];
    return;
  }
  /* position t P + e holds bin bin_of_pos; the row leaves in natural order, the band centre at N / 2 */
  float *nat = reinterpret_cast<float *>(wb);
  const float scale = 1.0f / (float)p.navg; /* a power of two: exact */
#pragma unroll
  for (int e = 0; e < P; e++) nat[(bin_of_pos<N, P>(t * P + e) + N / 2) & (N - 1)] = acc[e] * scale;
  wg_sync<NW>();
  float4 *out = reinterpret_cast<float4 *>(p.rows + (size_t)src * p.rows_stride + (size_t)unit * N);
#pragma unroll
  for (int m = 0; m < N / 4 / NT; m++) out[t + m * NT] = reinterpret_cast<const float4 *>(nat)[t + m * NT];
}

/* after the rows, in their stream: the pairs from the start of the first unfinished frame on -> the other history copy */
template <int N, int F>
__global__ void __launch_bounds__(256) rdsp_survey_finish_kernel(RdspSurveyParams p) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  const int src = blockIdx.y;
  if (m >= p.keep) return;
  const void *row = src_at<F>(p.src, (size_t)src * p.src_stride);
  p.hist_out[(size_t)src * N + m] = survey_pair<F>(row, p.hist_in + (size_t)src * N, p.keep_from + m, p.hist_len);
}

template <int N>
hipError_t survey_launch(int fmt, const RdspSurveyParams &p, int n_sources, int units, hipStream_t s) {
  return dispatch_format(fmt, [&](auto f) {
    constexpr int F = decltype(f)::value;
    if (units > 0) hipLaunchKernelGGL((rdsp_survey_kernel<N, F>), dim3(units, n_sources), dim3(N / SURVEY_P), 0, s, p);
    if (p.keep > 0) hipLaunchKernelGGL((rdsp_survey_finish_kernel<N, F>), dim3((p.keep + 255) / 256, n_sources), dim3(256), 0, s, p);
  });
}

uint64_t survey_frames(uint64_t t, uint64_t n) { return t < n ? 0u : (t - n) / (n / 2u) + 1u; }

}  // namespace

struct rdsp_survey {
  int n_sources, device, fft_n, navg, format;
  size_t max_pairs;
  uint64_t total = 0;            /* T: pairs per source since the last reset */
  int hist_cur = 0, part_cur = 0; /* which copy holds the history / the partial sums */
  rdsp_dev::DevBuf<float2> d_hist[2];
  rdsp_dev::DevBuf<float> d_part[2], d_window;
};

extern "C" int rdsp_survey_create(int n_sources, int device, int fft_n, int navg, int format, size_t max_pairs_per_call,
                                  rdsp_survey_t **out) {
  if (!out || n_sources < 1 || n_sources > 4096 || (fft_n != 1024 && fft_n != 4096) || navg < 1 || navg > 256 ||
      (navg & (navg - 1)) != 0 || format < 0 || format >= SRC_FORMATS || max_pairs_per_call < 1) {
    rdsp_set_error("rdsp_survey_create: 1 ... 4096 sources, fft_n 1024 or 4096, navg a power of two 1 ... 256, a format RDSP_SRC_*, "
                   "max_pairs_per_call at least 1");
    return RDSP_ERR_INVALID;
  }
  RC_TRY(rdsp_dev::need_device());
  std::vector<float> w((size_t)fft_n);
  RC_TRY(rdsp_survey_window(fft_n, w.data()));
  rdsp_survey_t *s = new rdsp_survey();
  s->n_sources = n_sources;
  s->device = device;
  s->fft_n = fft_n;
  s->navg = navg;
  s->format = format;
  s->max_pairs = max_pairs_per_call;
  const size_t n = (size_t)n_sources * (size_t)fft_n;
  bool ok = hipSetDevice(device) == hipSuccess && s->d_window.alloc((size_t)fft_n) == hipSuccess &&
            hipMemcpy(s->d_window, w.data(), (size_t)fft_n * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
  for (int i = 0; ok && i < 2; i++)
    ok = rdsp_dev::alloc_zero(s->d_hist[i], n) == hipSuccess && rdsp_dev::alloc_zero(s->d_part[i], n) == hipSuccess;
  if (!ok) {
    rdsp_set_error("rdsp_survey_create: device set-up failed");
    rdsp_survey_destroy(s);
    return RDSP_ERR_HIP;
  }
  *out = s;
  return RDSP_OK;
}
extern "C" void rdsp_survey_destroy(rdsp_survey_t *s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  delete s;
}
extern "C" int rdsp_survey_sources(const rdsp_survey_t *s) { return s ? s->n_sources : 0; }
extern "C" int rdsp_survey_fft_n(const rdsp_survey_t *s) { return s ? s->fft_n : 0; }
extern "C" int rdsp_survey_navg(const rdsp_survey_t *s) { return s ? s->navg : 0; }
extern "C" int rdsp_survey_format(const rdsp_survey_t *s) { return s ? s->format : -1; }
extern "C" int rdsp_survey_device(const rdsp_survey_t *s) { return s ? s->device : -1; }

extern "C" int rdsp_survey_reset(rdsp_survey_t *s, void *stream) {
  if (!s) {
    rdsp_set_error("rdsp_survey_reset: NULL object");
    return RDSP_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(s->device));
  const size_t n = (size_t)s->n_sources * (size_t)s->fft_n;
  for (int i = 0; i < 2; i++) {
    HIP_TRY(hipMemsetAsync(s->d_hist[i], 0, n * sizeof(float2), (hipStream_t)stream));
    HIP_TRY(hipMemsetAsync(s->d_part[i], 0, n * sizeof(float), (hipStream_t)stream));
  }
  s->total = 0;
  return RDSP_OK;
}

extern "C" int rdsp_survey_rows_for(const rdsp_survey_t *s, size_t pairs) {
  if (!s) return 0;
  return rdsp_survey_rows_between(s->fft_n, s->navg, s->total, pairs);
}

extern "C" int rdsp_survey_update(rdsp_survey_t *s, const void *d_src, size_t src_stride, size_t pairs, float *d_rows,
                                  size_t rows_stride, int *rows_out, void *stream) {
  if (!s) {
    rdsp_set_error("rdsp_survey_update: NULL object");
    return RDSP_ERR_INVALID;
  }
  if (pairs > s->max_pairs) {
    rdsp_set_error("rdsp_survey_update: %zu pairs, the object was created for calls of at most %zu", pairs, s->max_pairs);
    return RDSP_ERR_INVALID;
  }
  if (src_stride < pairs || (pairs > 0 && !d_src) || ((uintptr_t)d_src % (uintptr_t)src_pair_bytes(s->format)) != 0) {
    rdsp_set_error("rdsp_survey_update: source rows aligned to one pair (%d bytes), src_stride at least pairs", src_pair_bytes(s->format));
    return RDSP_ERR_INVALID;
  }
  const int rows = rdsp_survey_rows_between(s->fft_n, s->navg, s->total, pairs);
  if (rows < 0) return rows;
  if (rows_stride % 4 != 0 || ((uintptr_t)d_rows & 15u) != 0 || rows_stride < (size_t)rows * (size_t)s->fft_n || (rows > 0 && !d_rows)) {
    rdsp_set_error("rdsp_survey_update: the call completes %d rows: d_rows 16-byte aligned, rows_stride a multiple of 4 and at least %zu",
                   rows, (size_t)rows * (size_t)s->fft_n);
    return RDSP_ERR_INVALID;
  }
  if (rows_out) *rows_out = rows;
  if (pairs == 0) return RDSP_OK;
  HIP_TRY(hipSetDevice(s->device));
  const uint64_t n = (uint64_t)s->fft_n, h = n / 2u, navg = (uint64_t)s->navg;
  const uint64_t f0 = survey_frames(s->total, n), f1 = survey_frames(s->total + pairs, n);
  RdspSurveyParams p;
  memset(&p, 0, sizeof(p));
  p.src = d_src;
  p.src_stride = src_stride;
  p.hist_in = s->d_hist[s->hist_cur];
  p.hist_out = s->d_hist[s->hist_cur ^ 1];
  p.part_in = s->d_part[s->part_cur];
  p.part_out = s->d_part[s->part_cur ^ 1];
  p.window = s->d_window;
  p.rows = d_rows;
  p.rows_stride = rows_stride;
  p.hist_len = (int)(s->total - f0 * h); /* below N: frame f0 is unfinished */
  p.first = -(long long)p.hist_len;
  p.lead = (int)(f0 % navg);
  p.n_frames = (int)(f1 - f0);
  p.navg = s->navg;
  p.keep = (int)(s->total + pairs - f1 * h);
  p.keep_from = (long long)(f1 * h) - (long long)s->total; /* may lie before the call: pairs that stay in the history */
  const bool trailing = f1 > f0 && f1 % navg != 0; /* the call's last frames belong to a row it does not complete */
  const int units = f1 > f0 ? rows + (trailing ? 1 : 0) : 0;
  const hipError_t e = s->fft_n == 1024 ? survey_launch<1024>(s->format, p, s->n_sources, units, (hipStream_t)stream)
                                        : survey_launch<4096>(s->format, p, s->n_sources, units, (hipStream_t)stream);
  if (e != hipSuccess) {
    rdsp_set_error("rdsp_survey_update: kernel launch failed: %s", hipGetErrorString(e));
    return RDSP_ERR_HIP;
  }
  s->total += pairs;
  s->hist_cur ^= 1;
  if (trailing) s->part_cur ^= 1;
  return RDSP_OK;
}
