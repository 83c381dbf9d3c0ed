/*
 * rdsp_fft1024.hip -- AudioAnalyzeFFT1024 batched over channels (the second analyser of the
 * sketch's graph: `AudioAnalyzeFFT1024 AudioFFT;` fed from Q_out_L, RadioDSP_SDR_RX.ino:57,87,
 * read by the display).  The Teensy Audio library is not in the tree; its update() is restated
 * from the library's published behaviour: blocks are collected eight at a time and four
 * are kept (1024-sample frames, hop 512), the samples are real (imaginary parts zero), q15 window
 * (x*w) >> 15, arm_cfft_radix4_q15 as CMSIS publishes it (rdsp_q15.h),
 * output[i] = sqrt_uint32_approx(re^2 + im^2) for bins 0..511; window (AudioWindowHanning1024,
 * INO:147), twiddles and the square root's guess table are those of the reference's firmware
 * image (rdsp_q15_tables.c).  Integer arithmetic: bit-exact against the CPU restatement kept
 * with the tests.  The object's node is the analyser node of rdsp_graph_sdr.hip.
 *
 * One wave per channel.  Lane t runs the four butterflies b = t + 64 m of each of the five
 * stages (span L = 256, 64, 16, 4, 1); the packed int16 pairs go through a 4 KiB LDS buffer
 * between stages, the twiddle table W_1024^m sits in LDS too.  A frame reads 2 KiB of int16.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include "rdsp_host.h"
#include "rdsp_q15.h"
#include "rdsp_q15_host.h"
#include "rdsp_sync.h"

struct RdspFft1024Params {
  const int16_t *audio; /* [ch][in_stride] samples, every in_step int16 */
  size_t in_stride;
  int in_step;
  int n_new;            /* new samples in this call (n_blocks * 128) */
  int have;             /* samples already buffered per channel (0 .. 7*128), oldest first */
  int16_t *st_hist;     /* [ch][896] buffered samples */
  int n_frames;         /* frames completed by this call */
  int use_window;
  const int16_t *window;  /* [1024] q15 */
  const uint32_t *twid;   /* [768] cos | sin << 16 of 2 pi m / 1024 (rdsp_q15_twiddles) */
  const uint16_t *sqrt_guess; /* [33] */
  uint16_t *out;          /* [ch][out_stride][512] */
  size_t out_stride;
  int keep;             /* samples to buffer after this call */
};

namespace {
using namespace rdsp_q15;

/* sample `idx` of the channel's stream = [buffered history | this call's new samples] */
__device__ __forceinline__ int sample_at(const RdspFft1024Params &p, size_t ch, int idx) {
  if (idx < p.have) return p.st_hist[ch * 896 + idx];
  return p.audio[(ch * p.in_stride + (size_t)(idx - p.have)) * p.in_step];
}

__global__ void __launch_bounds__(64) rdsp_fft1024_kernel(RdspFft1024Params p) {
  __shared__ uint32_t ex[1024];
  __shared__ Twiddle tws[768]; /* W_1024^m as the two dot-product operands (rdsp_q15.h) */
  const int t = threadIdx.x;
  const size_t ch = blockIdx.x;
  for (int i = t; i < 768; i += 64) tws[i] = make_twiddle(p.twid[i]);
  wg_sync<1>();

  for (int f = 0; f < p.n_frames; f++) {
    const int base = 512 * f;
    /* stage 1 (span 256): butterfly b = t + 64 m takes positions b + 256 k straight from the
     * stream: copy_to_fft_buffer + window + the first radix-4 pass */
#pragma unroll
    for (int m = 0; m < 4; m++) {
      const int b = t + 64 * m;
      uint32_t x[4];
      Twiddle tw[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int pos = b + 256 * k;
        int v = sample_at(p, ch, base + pos);
        if (p.use_window) v = __mul24(v, (int)p.window[pos]) >> 15;
        x[k] = pack16(v, 0);
        if (k) tw[k] = tws[k * b]; /* j = b, n / (4 L) = 1; output 0 takes no twiddle */
      }
      bfly<kFirstStage>(x, tw);
#pragma unroll
      for (int k = 0; k < 4; k++) ex[b + 256 * k] = x[k];
    }
    wg_sync<1>();
    /* stages 2..5: span L = 64, 16, 4, 1 */
#pragma unroll
    for (int st = 1; st < 5; st++) {
      const int L = 256 >> (2 * st);
      uint32_t y[4][4];
#pragma unroll
      for (int m = 0; m < 4; m++) {
        const int b = t + 64 * m;
        const int g = (b / L) * 4 * L, j = b % L;
        Twiddle tw[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          y[m][k] = ex[g + j + k * L];
          if (k && L > 1) tw[k] = tws[k * j * (256 / L)];
        }
        if (L > 1) bfly<kMiddleStage>(y[m], tw);
        else bfly<kLastStage>(y[m], tw); /* no twiddles */
      }
      wg_sync<1>();
#pragma unroll
      for (int m = 0; m < 4; m++) {
        const int b = t + 64 * m;
        const int g = (b / L) * 4 * L, j = b % L;
#pragma unroll
        for (int k = 0; k < 4; k++) ex[g + j + k * L] = y[m][k];
      }
      wg_sync<1>();
    }
    /* position q holds bin digit-reverse_4(q) (five base-4 digits); bins 0..511 go out */
    uint16_t *o = p.out + (ch * p.out_stride + (size_t)f) * 512;
    for (int q = t; q < 1024; q += 64) {
      int bin = 0, r = q;
#pragma unroll
      for (int d = 0; d < 5; d++) { bin = (bin << 2) | (r & 3); r >>= 2; }
      if (bin < 512) {
        o[bin] = (uint16_t)sqrt_uint32_approx(magsq(ex[q]), p.sqrt_guess);
      }
    }
    wg_sync<1>();
  }
  /* the last `keep` samples of the stream stay buffered for the next call */
  const int total = p.have + p.n_new;
  int16_t tmp[14];
  int n_tmp = 0;
  for (int i = t; i < p.keep; i += 64) tmp[n_tmp++] = (int16_t)sample_at(p, ch, total - p.keep + i);
  wg_sync<1>(); /* every lane has read the old history before anyone overwrites it */
  n_tmp = 0;
  for (int i = t; i < p.keep; i += 64) p.st_hist[ch * 896 + i] = tmp[n_tmp++];
}
}  // namespace

/* ---- host side: struct rdsp_fft1024 and the tables' half are rdsp_q15_host.h's ------------- */
extern "C" int rdsp_fft1024_create(int n_channels, int device, int window_id, rdsp_fft1024_t **out) {
  if (!out || n_channels <= 0) {
    rdsp_set_error("rdsp_fft1024_create: bad argument");
    return RDSP_ERR_INVALID;
  }
  RC_TRY(rdsp_dev::need_device());
  return rdsp_q15_host::create(out, [&](rdsp_fft1024_t *s) {
    RC_TRY(s->init(n_channels, device, 1024, window_id));
    HIP_TRY(rdsp_dev::alloc_zero(s->d_hist, (size_t)n_channels * 896));
    return (int)RDSP_OK;
  });
}
extern "C" void rdsp_fft1024_destroy(rdsp_fft1024_t *s) { rdsp_q15_host::destroy(s); }
/* windowFunction by table name (INO:147), and windowFunction(const int16_t *w) with the library's own argument: a host
 * pointer to 1024 q15 taps (AudioWindowHanning1024) or NULL */
extern "C" int rdsp_fft1024_windowFunction(rdsp_fft1024_t *s, int window_id) { return rdsp_q15_host::public_set_window_id(s, window_id); }
extern "C" int rdsp_fft1024_windowFunction_table(rdsp_fft1024_t *s, const int16_t *w1024) { return rdsp_q15_host::public_set_window(s, w1024); }
/* AudioFFT.averageTogether(30) (INO:148): the library's 1024-point analyser declares it and does
 * nothing with it ("not implemented yet"); accepted and ignored here too */
extern "C" int rdsp_fft1024_averageTogether(rdsp_fft1024_t *s, int n) {
  (void)n;
  return s ? RDSP_OK : RDSP_ERR_INVALID;
}
/* frames the next update over n_blocks completes: the first after 8 blocks, then one per 4 */
extern "C" int rdsp_fft1024_outputs_for(const rdsp_fft1024_t *s, int n_blocks) {
  if (!s || n_blocks <= 0) return 0;
  const int total = s->have / 128 + n_blocks;
  return total < 8 ? 0 : (total - 8) / 4 + 1;
}
extern "C" int rdsp_fft1024_update(rdsp_fft1024_t *s, const int16_t *d_audio, size_t in_stride, int in_step, int n_blocks,
                                   uint16_t *d_out, size_t out_stride, int *n_outputs, void *stream) {
  if (!s || !d_audio || n_blocks <= 0 || in_step < 1 || in_stride < (size_t)n_blocks * 128) {
    rdsp_set_error("rdsp_fft1024_update: bad argument");
    return RDSP_ERR_INVALID;
  }
  const int nf = rdsp_fft1024_outputs_for(s, n_blocks);
  if (nf > 0 && (!d_out || out_stride < (size_t)nf)) {
    rdsp_set_error("rdsp_fft1024_update: output buffer holds %zu spectra per channel, %d needed", out_stride, nf);
    return RDSP_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(s->device));
  const int total = s->have + n_blocks * 128;
  RdspFft1024Params p;
  memset(&p, 0, sizeof(p));
  p.audio = d_audio;
  p.in_stride = in_stride;
  p.in_step = in_step;
  p.n_new = n_blocks * 128;
  p.have = s->have;
  p.st_hist = s->d_hist;
  p.n_frames = nf;
  p.use_window = s->has_window;
  p.window = s->d_window;
  p.twid = s->d_twid;
  p.sqrt_guess = s->d_guess;
  p.out = d_out;
  p.out_stride = out_stride;
  p.keep = nf > 0 ? total - 512 * nf : total; /* 4..7 blocks once frames run, everything before */
  hipLaunchKernelGGL(rdsp_fft1024_kernel, dim3(s->n_channels), dim3(64), 0, (hipStream_t)stream, p);
  RC_TRY(rdsp_q15_host::launched("fft1024"));
  s->have = p.keep;
  if (n_outputs) *n_outputs = nf;
  return RDSP_OK;
}
