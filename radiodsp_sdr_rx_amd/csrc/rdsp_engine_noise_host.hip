/* rdsp_engine_noise_host.hip -- the noise squelch of rdsp_engine_t on the host: EngNoise (rdsp_engine_host.h) owns the detector
 * words and the records, keeps the taps of every time constant it was run with and makes the launch; the entry points check their
 * arguments.  include/rdsp.h has the definition; the kernel is rdsp_engine_noise.hip's, the arithmetic rdsp_noise.h's.
 * rdsp_engine_update launches it per NFM group behind the group's meter, in front of its tone squelch. */
#include "rdsp_engine_host.h"

using namespace rdsp_noise;

hipError_t EngNoise::init(size_t n, size_t blocks_per_call) {
  n_channels = n; max_blocks = blocks_per_call;
  hipError_t err = alloc_zero(state, n * NOISE_WORDS);
  if (err == hipSuccess) err = alloc_zero(noise, n * max_blocks);
  if (err == hipSuccess) err = alloc_zero(nopen, n * max_blocks);
  return err;
}
hipError_t EngNoise::reset(hipStream_t s) { return hipMemsetAsync(state, 0, n_channels * NOISE_WORDS * 4, s); }
const float *EngNoise::taps_of(float tau_us) {
  for (const Taps &t : taps)
    if (t.tau_us == tau_us) return t.g;
  if (taps.size() >= 16) taps.clear(); /* a caller that sweeps the time constant */
  taps.emplace_back(); /* a group's set_fm changed, or the first call: the taps belong to the time constant */
  taps.back().tau_us = tau_us;
  noise_taps(tau_us, taps.back().g);
  return taps.back().g;
}
hipError_t EngNoise::launch_group(const EngParams &p, size_t c0, const NoiseSet &set, const rdsp_fm::FmSet &fm, const EngMeter *meter,
                                  const int16_t *d_lr, hipStream_t s) {
  if (set.mode == NOISE_OFF) /* the group's words are zeros, its records read zeros: no launch */
    return hipMemsetAsync(state + c0 * NOISE_WORDS, 0, (size_t)p.n_channels * NOISE_WORDS * 4, s);
  NoiseParams t{};
  t.audio = p.audio; t.audio_stride = p.audio_stride; t.out = p.out; t.out_stride = p.out_stride;
  t.out_vec = ((uintptr_t)d_lr & 15) == 0 && p.out_stride % 4 == 0;
  t.n_channels = p.n_channels; t.n_blocks = p.n_blocks; t.reset = (p.resets & RESET_FM) != 0;
  t.key = noise_key(set.mode, fm.W, fm.tau_us != 0.0f);
  t.set = set;
  t.state = state + c0 * NOISE_WORDS;
  t.rec_stride = max_blocks; t.noise = noise + c0 * max_blocks; t.nopen = nopen + c0 * max_blocks;
  if (meter && set.mode == NOISE_GATE) {
    t.open = meter->open + c0 * meter->max_blocks; t.open_stride = meter->max_blocks; t.meter_words = meter->words + c0 * MT_WORDS;
  }
  memcpy(t.taps, taps_of(fm.tau_us), NOISE_TAPS * sizeof(float));
  const hipError_t err = rdsp_engine_noise_launch(t, s);
  if (err == hipSuccess) rows.emplace_back(c0, (size_t)p.n_channels); /* only rows a launch wrote are read_noise's */
  return err;
}

extern "C" {

int rdsp_engine_noise_taps(float tau_us, float *out) {
  if (!out || !rdsp_fm::tau_ok(tau_us)) {
    rdsp_set_error("rdsp_engine_noise_taps: bad argument (tau_us %g of 0 or 25 .. 1000; out not NULL)", (double)tau_us);
    return RDSP_ERR_INVALID;
  }
  noise_taps(tau_us, out);
  return RDSP_OK;
}

int rdsp_engine_enable_noise(rdsp_engine_t *e) {
  if (!e) return RDSP_ERR_INVALID;
  if (e->noise) return RDSP_OK;
  if (!e->fm) {
    rdsp_set_error("rdsp_engine_enable_noise: the noise squelch runs on narrow-band FM receivers; call rdsp_engine_enable_fm first");
    return RDSP_ERR_NOT_READY;
  }
  auto t = std::make_unique<EngNoise>(); /* the object stays without the detector unless all of it exists */
  hipError_t err = hipSetDevice(e->device);
  if (err == hipSuccess) err = hipDeviceSynchronize(); /* the next call of every stream may run it */
  if (err == hipSuccess) err = t->init((size_t)e->n_channels, (size_t)e->max_blocks);
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err != hipSuccess) {
    rdsp_set_error("rdsp_engine_enable_noise: %s", hipGetErrorString(err));
    return RDSP_ERR_NOMEM;
  }
  e->noise = std::move(t);
  return RDSP_OK;
}
int rdsp_engine_noise_enabled(const rdsp_engine_t *e) { return e && e->noise ? 1 : 0; }

int rdsp_engine_set_noise_squelch(rdsp_engine_t *e, int mode, float open_n, float close_n, int hang_blocks, float fall, float rise) {
  if (!e || !squelch_ok(mode, open_n, close_n, hang_blocks, fall, rise)) {
    rdsp_set_error("rdsp_engine_set_noise_squelch: bad argument (mode %d of 0 .. 2; 0 < open_n %g <= close_n %g, finite; hang_blocks %d of 0 .. %d; "
                   "fall %g and rise %g of (0, 1])", mode, (double)open_n, (double)close_n, hang_blocks, rdsp_meter::HANG_MAX, (double)fall, (double)rise);
    return RDSP_ERR_INVALID;
  }
  return for_selected(e, [&](EngSettings &s) { s.noise = {mode, open_n, close_n, hang_blocks, fall, rise}; });
}

int rdsp_engine_read_noise(rdsp_engine_t *e, int n_blocks, float *d_noise, size_t noise_stride, uint8_t *d_open, size_t open_stride, void *stream) {
  if (!e) return RDSP_ERR_INVALID;
  if (!e->noise) {
    rdsp_set_error("rdsp_engine_read_noise: the noise squelch is off; call rdsp_engine_enable_noise first");
    return RDSP_ERR_NOT_READY;
  }
  const size_t w = (size_t)std::max(n_blocks, 0);
  if (n_blocks < 0 || n_blocks > e->last_blocks || (d_noise && noise_stride < w) || (d_open && open_stride < w)) {
    rdsp_set_error("rdsp_engine_read_noise: bad argument (n_blocks %d of the last call's %d; strides at least n_blocks)", n_blocks, e->last_blocks);
    return RDSP_ERR_INVALID;
  }
  if (w == 0) return RDSP_OK;
  const EngNoise &t = *e->noise;
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)e->n_channels;
  hipError_t err = hipSetDevice(e->device);
  /* receivers the detector did not run on: zeros */
  if (err == hipSuccess && d_noise) err = hipMemset2DAsync(d_noise, noise_stride * 4, 0, w * 4, n, s);
  if (err == hipSuccess && d_open) err = hipMemset2DAsync(d_open, open_stride, 0, w, n, s);
  for (size_t k = 0; k < t.rows.size() && err == hipSuccess; k++) {
    const size_t c0 = t.rows[k].first, count = t.rows[k].second, mb = t.max_blocks;
    if (d_noise) err = hipMemcpy2DAsync(d_noise + c0 * noise_stride, noise_stride * 4, t.noise + c0 * mb, mb * 4, w * 4, count, hipMemcpyDeviceToDevice, s);
    if (err == hipSuccess && d_open) err = hipMemcpy2DAsync(d_open + c0 * open_stride, open_stride, t.nopen + c0 * mb, mb, w, count, hipMemcpyDeviceToDevice, s);
  }
  return err == hipSuccess ? RDSP_OK : engine_fail("rdsp_engine_read_noise", err);
}

}  // extern "C"
