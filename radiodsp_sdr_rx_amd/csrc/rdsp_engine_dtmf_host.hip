/* rdsp_engine_dtmf_host.hip -- the DTMF decoder of rdsp_engine_t on the host: EngDtmf (rdsp_engine_host.h) owns the detector
 * words, the records and its copy of the phasor table and makes the launch; the entry points check their arguments.
 * include/rdsp.h has the definition; the kernel is rdsp_engine_dtmf.hip's, the arithmetic rdsp_dtmf.h's.  rdsp_engine_update
 * launches it per NFM group with a frame length behind the group's other detectors. */
#include "rdsp_engine_host.h"

using namespace rdsp_dtmf;

hipError_t EngDtmf::init(size_t n, size_t blocks_per_call) {
  n_channels = n; max_blocks = blocks_per_call;
  hipError_t err = alloc_zero(state, n * DTMF_WORDS);
  if (err == hipSuccess) err = alloc_zero(key, n * max_blocks);
  if (err == hipSuccess) err = alloc_zero(fresh, n * max_blocks);
  if (err == hipSuccess) err = alloc_zero(lo, n * max_blocks);
  if (err == hipSuccess) err = alloc_zero(hi, n * max_blocks);
  if (err == hipSuccess) err = tab.alloc(rdsp_tune::TUNE_N);
  if (err == hipSuccess) err = hipMemcpy(tab, rdsp_engine_tune_table(), rdsp_tune::TUNE_N * sizeof(float4), hipMemcpyHostToDevice);
  return err;
}
hipError_t EngDtmf::reset(hipStream_t s) { return hipMemsetAsync(state, 0, n_channels * DTMF_WORDS * 4, s); }
hipError_t EngDtmf::launch_group(const EngParams &p, size_t c0, const DtmfSet &set, hipStream_t s) {
  DtmfParams t{};
  t.audio = p.audio; t.audio_stride = p.audio_stride;
  t.n_channels = p.n_channels; t.n_blocks = p.n_blocks; t.reset = (p.resets & RESET_FM) != 0;
  t.law = dtmf_law(set);
  t.tab = tab; t.state = state + c0 * DTMF_WORDS;
  t.rec_stride = max_blocks; t.key = key + c0 * max_blocks; t.fresh = fresh + c0 * max_blocks; t.lo = lo + c0 * max_blocks; t.hi = hi + c0 * max_blocks;
  const hipError_t err = rdsp_engine_dtmf_launch(t, s);
  if (err == hipSuccess) rows.emplace_back(c0, (size_t)p.n_channels); /* only rows a launch wrote are read_dtmf's */
  return err;
}
hipError_t EngDtmf::clear_group(size_t c0, size_t count, hipStream_t s) {
  return hipMemsetAsync(state + c0 * DTMF_WORDS, 0, count * DTMF_WORDS * 4, s);
}

extern "C" {

char rdsp_engine_dtmf_key(int sym) { return dtmf_key(sym); }

double rdsp_engine_dtmf_gain(float hz, float tau_us) {
  if (!(hz > 0.0f && hz < (float)rdsp_tune::TUNE_MAX_HZ) || !rdsp_fm::tau_ok(tau_us)) {
    rdsp_set_error("rdsp_engine_dtmf_gain: bad argument (hz %g of (0, 22050); tau_us %g of 0 or 25 .. 1000)", (double)hz, (double)tau_us);
    return 0.0;
  }
  return dtmf_boxcar_gain(hz) * rdsp_engine_tone_gain(hz, tau_us);
}

int rdsp_engine_enable_dtmf(rdsp_engine_t *e) {
  if (!e) return RDSP_ERR_INVALID;
  if (e->dtmf) return RDSP_OK;
  if (!e->fm) {
    rdsp_set_error("rdsp_engine_enable_dtmf: the DTMF decoder runs on narrow-band FM receivers; call rdsp_engine_enable_fm first");
    return RDSP_ERR_NOT_READY;
  }
  auto t = std::make_unique<EngDtmf>(); /* the object stays without the decoder unless all of it exists */
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess) err = hipDeviceSynchronize(); /* the next call of every stream may run it */
  if (err == hipSuccess) err = t->init((size_t)e->n_channels, (size_t)e->max_blocks);
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err != hipSuccess) {
    rdsp_set_error("rdsp_engine_enable_dtmf: %s", hipGetErrorString(err));
    return RDSP_ERR_NOMEM;
  }
  e->dtmf = std::move(t);
  return RDSP_OK;
}
int rdsp_engine_dtmf_enabled(const rdsp_engine_t *e) { return e && e->dtmf ? 1 : 0; }

int rdsp_engine_set_dtmf(rdsp_engine_t *e, int K, float min_amp, float ratio, float twist, float share, int on_frames, int off_frames) {
  if (!e || !dtmf_ok(K, min_amp, ratio, twist, share, on_frames, off_frames)) {
    rdsp_set_error("rdsp_engine_set_dtmf: bad argument (K %d of 0 or %d .. %d; 0 < min_amp %g <= 1; 1 <= ratio %g <= 1e6; 1 <= twist %g <= 1e6; "
                   "0 < share %g <= 1; on_frames %d and off_frames %d of 1 .. %d)",
                   K, DTMF_MIN_K, DTMF_MAX_K, (double)min_amp, (double)ratio, (double)twist, (double)share, on_frames, off_frames, DTMF_MAX_FRAMES);
    return RDSP_ERR_INVALID;
  }
  return for_selected(e, [&](EngSettings &s) { s.dtmf = {K, min_amp, ratio, twist, share, on_frames, off_frames}; });
}

int rdsp_engine_read_dtmf(rdsp_engine_t *e, int n_blocks, uint8_t *d_key, size_t key_stride, uint8_t *d_new, size_t new_stride, float *d_lo,
                          size_t lo_stride, float *d_hi, size_t hi_stride, void *stream) {
  if (!e) return RDSP_ERR_INVALID;
  if (!e->dtmf) {
    rdsp_set_error("rdsp_engine_read_dtmf: the DTMF decoder is off; call rdsp_engine_enable_dtmf first");
    return RDSP_ERR_NOT_READY;
  }
  const size_t w = (size_t)std::max(n_blocks, 0);
  if (n_blocks < 0 || n_blocks > e->last_blocks || (d_key && key_stride < w) || (d_new && new_stride < w) || (d_lo && lo_stride < w) ||
      (d_hi && hi_stride < w)) {
    rdsp_set_error("rdsp_engine_read_dtmf: bad argument (n_blocks %d of the last call's %d; strides at least n_blocks)", n_blocks, e->last_blocks);
    return RDSP_ERR_INVALID;
  }
  if (w == 0) return RDSP_OK;
  const EngDtmf &t = *e->dtmf;
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)e->n_channels;
  hipError_t err = hipSetDevice(e->device);
  /* receivers the decoder did not run on: none, none, 0, 0 */
  if (err == hipSuccess && d_key) err = hipMemset2DAsync(d_key, key_stride, (int)DTMF_NONE, w, n, s);
  if (err == hipSuccess && d_new) err = hipMemset2DAsync(d_new, new_stride, (int)DTMF_NONE, w, n, s);
  if (err == hipSuccess && d_lo) err = hipMemset2DAsync(d_lo, lo_stride * 4, 0, w * 4, n, s);
  if (err == hipSuccess && d_hi) err = hipMemset2DAsync(d_hi, hi_stride * 4, 0, w * 4, n, s);
  for (size_t k = 0; k < t.rows.size() && err == hipSuccess; k++) {
    const size_t c0 = t.rows[k].first, count = t.rows[k].second, mb = t.max_blocks;
    if (d_key) err = hipMemcpy2DAsync(d_key + c0 * key_stride, key_stride, t.key + c0 * mb, mb, w, count, hipMemcpyDeviceToDevice, s);
    if (err == hipSuccess && d_new) err = hipMemcpy2DAsync(d_new + c0 * new_stride, new_stride, t.fresh + c0 * mb, mb, w, count, hipMemcpyDeviceToDevice, s);
    if (err == hipSuccess && d_lo) err = hipMemcpy2DAsync(d_lo + c0 * lo_stride, lo_stride * 4, t.lo + c0 * mb, mb * 4, w * 4, count, hipMemcpyDeviceToDevice, s);
    if (err == hipSuccess && d_hi) err = hipMemcpy2DAsync(d_hi + c0 * hi_stride, hi_stride * 4, t.hi + c0 * mb, mb * 4, w * 4, count, hipMemcpyDeviceToDevice, s);
  }
  return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_read_dtmf", err);
}

int rdsp_engine_read_dtmf_digits(rdsp_engine_t *e, int first_channel, int n_channels, uint32_t *d_count, uint32_t *d_ring, void *stream) {
  if (!e) return RDSP_ERR_INVALID;
  if (!e->dtmf) {
    rdsp_set_error("rdsp_engine_read_dtmf_digits: the DTMF decoder is off; call rdsp_engine_enable_dtmf first");
    return RDSP_ERR_NOT_READY;
  }
  if (first_channel < 0 || n_channels < 1 || n_channels > e->n_channels - first_channel) {
    rdsp_set_error("rdsp_engine_read_dtmf_digits: bad argument (channels %d .. of %d)", first_channel, e->n_channels);
    return RDSP_ERR_INVALID;
  }
  const uint32_t *w = e->dtmf->state + (size_t)first_channel * DTMF_WORDS;
  hipStream_t s = (hipStream_t)stream;
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess && d_count) err = hipMemcpy2DAsync(d_count, 4, w + DT_NDIGITS, DTMF_WORDS * 4, 4, (size_t)n_channels, hipMemcpyDeviceToDevice, s);
  if (err == hipSuccess && d_ring)
    err = hipMemcpy2DAsync(d_ring, RING * 4, w + DT_RING, DTMF_WORDS * 4, RING * 4, (size_t)n_channels, hipMemcpyDeviceToDevice, s);
  return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_read_dtmf_digits", err);
}

}  // extern "C"
