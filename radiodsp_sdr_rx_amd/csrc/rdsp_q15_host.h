/*
 * rdsp_q15_host.h -- the host half that the two integer analysers share (rdsp_spectrum.hip, N = 256; rdsp_fft1024.hip,
 * N = 1024): the channel count, the device and the three device tables -- a q15 window of N taps, 3N/4 packed twiddles,
 * the 33 root guesses -- with their set-up, the two windowFunction() forms, the check behind a launch, and create /
 * destroy of an object made of it.  The two objects are defined here because the analyser node (rdsp_graph_sdr.hip) reads
 * their channel count and device.  (The refusal on a machine without a device, which the biquad and the survey share, is
 * rdsp_dev::need_device.)
 */
#ifndef RDSP_Q15_HOST_H
#define RDSP_Q15_HOST_H

#include <vector>

#include "rdsp_dev.h"

namespace rdsp_q15_host {

struct Q15Host {
  int n_channels = 0, device = 0, N = 0;
  int has_window = 0; /* `const int16_t *window` non-NULL, FFTIQ.h:101, FFTIQ.cpp:81 */
  rdsp_dev::DevBuf<int16_t> d_window;
  rdsp_dev::DevBuf<uint16_t> d_guess;
  rdsp_dev::DevBuf<uint32_t> d_twid;

  /* makes the device current (the caller's allocations follow on it) */
  int init(int nch, int dev, int n, int window_id) {
    n_channels = nch;
    device = dev;
    N = n;
    std::vector<uint32_t> tw((size_t)(3 * n / 4));
    rdsp_q15_twiddles(n, tw.data());
    HIP_TRY(hipSetDevice(dev));
    HIP_TRY(d_window.alloc((size_t)n));
    HIP_TRY(d_twid.alloc(tw.size()));
    HIP_TRY(d_guess.alloc(33));
    HIP_TRY(hipMemcpy(d_twid, tw.data(), tw.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_guess, rdsp_sqrt_guess_table(), 33 * sizeof(uint16_t), hipMemcpyHostToDevice));
    return set_window_id(window_id);
  }
  /* windowFunction(const int16_t *w), FFTIQ.h:93-95: the analyser keeps the caller's table of N taps (a copy here: the
   * table lives in device memory); NULL switches the window off (FFTIQ.cpp:81) */
  int set_window(const int16_t *w) {
    has_window = w != nullptr;
    if (w) HIP_TRY(hipMemcpy(d_window, w, (size_t)N * sizeof(int16_t), hipMemcpyHostToDevice));
    return RDSP_OK;
  }
  int set_window_id(int window_id) {
    if (window_id == RDSP_WINDOW_NONE) return set_window(nullptr);
    if (window_id < 0 || window_id > RDSP_WINDOW_TUKEY) {
      rdsp_set_error("unknown window id %d", window_id);
      return RDSP_ERR_INVALID;
    }
    std::vector<int16_t> w((size_t)N);
    rdsp_window_q15_n(window_id, N, w.data());
    return set_window(w.data());
  }
  /* in front of a public window setter: an update that reads the old table may still be running */
  int wait() {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipDeviceSynchronize());
    return RDSP_OK;
  }
};

/* the public windowFunction() pair of an analyser */
static inline int public_set_window_id(Q15Host *s, int window_id) {
  if (!s) return RDSP_ERR_INVALID;
  RC_TRY(s->wait());
  return s->set_window_id(window_id);
}
static inline int public_set_window(Q15Host *s, const int16_t *w) {
  if (!s) return RDSP_ERR_INVALID;
  RC_TRY(s->wait());
  return s->set_window(w);
}

/* behind an analyser's kernel launch */
static inline int launched(const char *who) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return RDSP_OK;
  rdsp_set_error("%s kernel launch failed: %s", who, hipGetErrorString(e));
  return RDSP_ERR_HIP;
}

template <typename T>
void destroy(T *s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  delete s;
}
/* a new T set up by setup(T *): a refusal or a failed HIP call (RDSP_ERR_HIP, the text of HIP_TRY) destroys the half-made
 * object and is returned */
template <typename T, typename Setup>
int create(T **out, Setup setup) {
  T *s = new T();
  const int rc = setup(s);
  if (rc != RDSP_OK) {
    destroy(s);
    return rc;
  }
  *out = s;
  return RDSP_OK;
}

}  // namespace rdsp_q15_host

/* AudioAnalyzeFFT256IQ: what is its own besides the tables (rdsp_spectrum.hip) */
struct rdsp_spectrum : rdsp_q15_host::Q15Host {
  int naverage = 1;
  int have_prev = 0, count = 0;
  rdsp_dev::DevBuf<uint32_t> d_prev, d_sum; /* [ch][128] previous block, [ch][256] sum[] */
};
/* AudioAnalyzeFFT1024 (rdsp_fft1024.hip) */
struct rdsp_fft1024 : rdsp_q15_host::Q15Host {
  int have = 0; /* samples buffered per channel */
  rdsp_dev::DevBuf<int16_t> d_hist; /* [ch][896] */
};
#endif
