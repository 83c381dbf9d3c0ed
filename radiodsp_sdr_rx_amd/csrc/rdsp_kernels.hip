/*
 * rdsp_kernels.hip -- the launch layer of the front kernels and the chain's small kernels (gfx950).
 *
 *   rdsp_front_pick      which front-kernel instance a call runs: family, LEAN, PRE, Q4, frame length.  The one
 *                        statement of that choice -- the chain's timing records take the kernel's name from it too
 *   rdsp_launch_front    launches what it names, through the family's entry (rdsp_front_launch.h)
 *   rdsp_group_store_kernel, rdsp_iq_slip_kernel, rdsp_q15_to_float_kernel, rdsp_float_to_q15_kernel
 *                        with their launchers
 *
 * The front kernels themselves: rdsp_front_direct.hip (rdsp_front_kernel: decimator in direct form, or none),
 * rdsp_front_fd.hip (rdsp_front_fd_kernel: frequency domain, wave-wide frames), rdsp_front_rd.hip
 * (rdsp_front_rd_kernel: frequency domain, 16-lane rows); what they share behind the decimator: rdsp_front_frame.h.
 * The tail kernels: rdsp_tail.hip, rdsp_tail_engine.hip; the SAM demodulator: rdsp_sam.hip.
 */
#include <stdlib.h>
#include <string.h>

#include "rdsp_front.h"
#include "rdsp_front_launch.h"

using namespace rdsp;

namespace {

/* one group record, rewritten in stream order (32 threads, one dword each) */
struct RdspGroupWords { uint32_t w[32]; };
__global__ void rdsp_group_store_kernel(uint32_t *dst, RdspGroupWords v) { dst[threadIdx.x] = v.w[threadIdx.x]; }

/* ---- pre-processor: I2S channel-slip correction (rdsp_pre_setIQslip) -------------------------
 * One rail of the stream is a sample behind the other: the corrected word pairs this sample's half
 * of one rail with the previous sample's half of the other (slip +1: I[n-1] | Q[n], slip -1:
 * I[n] | Q[n-1]).  A pass of its own in front of the front kernel, over the raw words: 8 bytes of HBM
 * traffic per input sample while the correction is on, nothing when it is off; the front kernels and
 * the 256-sample FIR history see corrected words only.  carry_in[ch * carry_stride]: the last raw word
 * of the previous call -- the chain's FIR history when that call ran without the correction, else the
 * word the previous pass left in carry_out (two arrays, alternating: every thread's predecessor word
 * is read before any carry is written). */
__global__ void __launch_bounds__(256) rdsp_iq_slip_kernel(const uint32_t *in, size_t in_stride, uint32_t *out,
                                                           size_t out_stride, const uint32_t *carry_in, size_t carry_stride,
                                                           uint32_t *carry_out, int n_quads, int slip) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  const size_t ch = blockIdx.y;
  if (q >= n_quads) return;
  const uint32_t *src = in + ch * in_stride;
  const uint4 w = *reinterpret_cast<const uint4 *>(src + 4 * (size_t)q);
  const uint32_t p = (q == 0) ? carry_in[ch * carry_stride] : src[4 * (size_t)q - 1];
  const uint32_t lo = 0x0000FFFFu;
  uint4 r;
  if (slip > 0) { /* I of the previous sample, Q of this one */
    r.x = (p & lo) | (w.x & ~lo); r.y = (w.x & lo) | (w.y & ~lo); r.z = (w.y & lo) | (w.z & ~lo); r.w = (w.z & lo) | (w.w & ~lo);
  } else {        /* I of this sample, Q of the previous one */
    r.x = (w.x & lo) | (p & ~lo); r.y = (w.y & lo) | (w.x & ~lo); r.z = (w.z & lo) | (w.y & ~lo); r.w = (w.w & lo) | (w.z & ~lo);
  }
  *reinterpret_cast<uint4 *>(out + ch * out_stride + 4 * (size_t)q) = r;
  if (q == n_quads - 1) carry_out[ch] = w.w;
}

/* ---- standalone A1 / A10 (bit-exact tests of the int16 <-> float edges) ---- */
__global__ void rdsp_q15_to_float_kernel(const int16_t *src, float *dst, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) dst[i] = (float)src[i] * (1.0f / 32768.0f);
}
__global__ void rdsp_float_to_q15_kernel(const float *src, int16_t *dst, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) dst[i] = (int16_t)q15_of_float(src[i]);
}

}  // namespace

/* LEAN = true trades registers for a little recomputation; it pays at radix 16, where it buys the second wave per SIMD,
 * and is selectable below that (rdsp_chain_set_front_variant).  On 16-lane rows the plan's radix decides: the rows need
 * the registers, the `lean` switch is for the wave-wide forms.
 * PRE: blanker, swap, a FIR history that came in under another swap flag / other input gains, or different gains on I
 * and Q (iq_balance) -- the kernels without PRE fold the one gain into the mixer.
 * fir_fd 1: 448-sample frames (throughput form, fir_variant 2); 2: one granule per frame (split-invariant); 3: the
 * row form, 128 outputs per window -- with the noise blanker on, the wave-wide form with the same split behaviour (2):
 * its decisions travel with the raw words from frame to frame.  fir_fd 4 (192 outputs per window) and fir_matrix (the
 * decimating FIR on the matrix cores) were measured and not adopted (docs/history.md): not supported.
 * Q4, FFT_L 256: four overlap-save frames per pass (front_frame_quad) unless the audio goes on to the tail kernel, which
 * may share the SIMDs (pipelined mode) and leaves no room for that form's registers and LDS.  Measurement switch
 * RDSP_NO_QUAD=1: the one-frame form behind the wave-wide decimator too (tests/micro/k2_occupancy.sh). */
extern "C" int rdsp_front_pick(int fft_l, int decim, const RdspFrontParams *p, RdspFrontPick *pick) {
  if (decim != 1 && decim != 4) return (int)hipErrorInvalidValue;
  RdspFrontPick k = {};
  k.radix = with_front_plan(fft_l, 0, [](auto plan) { return decltype(plan)::P; });
  if (!k.radix) return (int)hipErrorInvalidValue;
  k.lean = k.radix == 16 || p->lean;
  const bool hist_differs = p->swap_hist != p->swap_iq || p->scale_i_hist != p->scale_i || p->scale_q_hist != p->scale_q;
  k.pre = p->nb_on || p->swap_iq || hist_differs || p->scale_i != p->scale_q;
  const bool one_hop_frames = fft_l == 256 && !p->to_mid; /* room for front_frame_quad */
  if (decim == 4 && p->fir_fd) {
    if (p->fir_fd >= 3 && !p->nb_on) {
      if (!p->rd_mask) return (int)hipErrorInvalidValue;
      if (p->fir_fd == 4) return (int)hipErrorNotSupported;
      k.family = RDSP_FRONT_RD;
      k.lean = k.radix >= 8;
      k.frame = 128;
      k.q4 = one_hop_frames;
    } else {
      static const bool no_quad = getenv("RDSP_NO_QUAD") && atoi(getenv("RDSP_NO_QUAD")) != 0;
      k.family = RDSP_FRONT_FD;
      k.frame = (p->fir_fd == 2 || p->fir_fd == 3) ? 4 : RDSP_FD_P - 1;
      k.q4 = one_hop_frames && !no_quad;
    }
  } else {
    if (p->fir_matrix) return (int)hipErrorNotSupported;
    k.family = RDSP_FRONT_DIRECT;
  }
  *pick = k;
  return 0;
}

/* ROTG, inside the wave-wide frequency-domain family: the chain hands over a pool of per-group rotated branch spectra
 * while it has at most RDSP_FD_ROT_GROUPS groups (chain_groups_resize), and with one the instances that read it run */
extern "C" int rdsp_front_pick_rotg(const RdspFrontParams *p) { return p->rot_pool != nullptr; }

/* SHF, inside ROTG: the NCO behind the decimator, on a quarter of the samples, the pool holding the spectra of the
 * frequency-shifted taps.  The one-wave plans take it; the four-wave plans (FFT_L >= 2048) keep the rotated spectra: a
 * run-time form of this lost there once (docs/history.md) and this form has not been timed on K4.  The chain fills the pool
 * by the same rule (rdsp_fd_shift_plan) and says so in fd_shift. */
extern "C" int rdsp_fd_shift_plan(int fft_l) { return fft_l <= 1024; }
extern "C" int rdsp_front_pick_shift(int fft_l, const RdspFrontParams *p) {
  return rdsp_front_pick_rotg(p) && p->fd_shift && rdsp_fd_shift_plan(fft_l);
}

extern "C" const char *rdsp_front_kernel_name(int family) {
  return family == RDSP_FRONT_RD ? "rdsp_front_rd_kernel" : (family == RDSP_FRONT_FD ? "rdsp_front_fd_kernel" : "rdsp_front_kernel");
}

extern "C" int rdsp_launch_front(int fft_l, int decim, const RdspFrontParams *p, int n_channels,
                                 hipStream_t stream) {
  RdspFrontPick k;
  const int e = rdsp_front_pick(fft_l, decim, p, &k);
  if (e != 0) return e;
  switch (k.family) {
    case RDSP_FRONT_RD: return front_rd_launch(fft_l, k, p, n_channels, stream);
    case RDSP_FRONT_FD: return front_fd_launch(fft_l, k, p, n_channels, stream);
    default: return front_direct_launch(fft_l, decim, k, p, n_channels, stream);
  }
}

extern "C" int rdsp_launch_group_store(RdspGroup *dst, const RdspGroup *val, hipStream_t stream) {
  static_assert(sizeof(RdspGroup) == 128, "group record is 32 dwords");
  RdspGroupWords v;
  memcpy(&v, val, sizeof(v));
  hipLaunchKernelGGL(rdsp_group_store_kernel, dim3(1), dim3(32), 0, stream, reinterpret_cast<uint32_t *>(dst), v);
  return (int)hipGetLastError();
}

extern "C" int rdsp_launch_iq_slip(const uint32_t *in, size_t in_stride, uint32_t *out, size_t out_stride,
                                   const uint32_t *carry_in, size_t carry_stride, uint32_t *carry_out, int n_samples,
                                   int slip, int n_channels, hipStream_t stream) {
  const int nq = n_samples / 4;
  hipLaunchKernelGGL(rdsp_iq_slip_kernel, dim3((nq + 255) / 256, n_channels), dim3(256), 0, stream, in, in_stride, out,
                     out_stride, carry_in, carry_stride, carry_out, nq, slip);
  return (int)hipGetLastError();
}

extern "C" int rdsp_launch_q15_to_float(const int16_t *src, float *dst, size_t n, hipStream_t stream) {
  int grid = (int)((n + 255) / 256);
  if (grid > 4096) grid = 4096;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(rdsp_q15_to_float_kernel, dim3(grid), dim3(256), 0, stream, src, dst, n);
  return (int)hipGetLastError();
}
extern "C" int rdsp_launch_float_to_q15(const float *src, int16_t *dst, size_t n, hipStream_t stream) {
  int grid = (int)((n + 255) / 256);
  if (grid > 4096) grid = 4096;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(rdsp_float_to_q15_kernel, dim3(grid), dim3(256), 0, stream, src, dst, n);
  return (int)hipGetLastError();
}
